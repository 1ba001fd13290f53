"""Variable-coefficient operators on the device: the fused weighted assembly (`assemble_weighted_kernel`) bit for bit and entry
by entry, posteriors against a dense NumPy/SciPy reference built from the oracle's constant-coefficient blocks
(tests/_varcoef_reference.py), what reads the factor afterwards, and every refusal."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import _varcoef_reference as vr
from conftest import POSTERIOR_RTOL, posterior_tolerances
from oracle import covfuncs as ocf

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.double).eps)
ENTRY_RTOL = 1e-13           # tests/test_gpu_kernels.py: |K - oracle| <= 1e-13 max|oracle| for unweighted blocks of these descriptors


@pytest.fixture(scope="module")
def lp():
    import linpde_gp_amd
    return linpde_gp_amd


@pytest.fixture(scope="module")
def ctx(lp):
    from linpde_gp_amd import _engine
    return _engine.default_context()


def _two_block_matrix(ctx, P0, P1, k00):
    """A matrix of two blocks (70 and 130 rows) whose block (0, 0) is assembled: blocks (1, 0), 130 x 70, and (1, 1) are the test's."""
    from linpde_gp_amd import _engine
    M = _engine.GramMatrix(ctx)
    M.add_block(P0.n)
    M.add_block(P1.n)
    M.assemble(k00, P0, None, 0, 0)
    return M


def _descriptor_cases(lp):
    from linpde_gp_amd.linfuncops import diffops
    cf = lp.randprocs.covfuncs
    out = []
    for d in (1, 2, 3):
        k = 1.7 * (cf.TensorProduct(*[cf.Matern((), nu=2.5, lengthscales=0.6 + 0.3 * j) for j in range(d)]) if d > 1 else cf.Matern((1,), nu=2.5, lengthscales=0.6))
        Lap = -1.0 * diffops.Laplacian((d,))
        out.append((f"product Matern-5/2, d={d}, Laplacian on both sides", d, k, Lap(Lap(k, argnum=1), argnum=0)))
    kiso = cf.Matern((2,), nu=2.5, lengthscales=[0.7, 1.1])
    Dv, Dw = diffops.DirectionalDerivative([1.0, -0.5]), diffops.DirectionalDerivative([0.3, 2.0])
    out.append(("isotropic Matern-5/2, d=2, directional derivatives", 2, kiso, Dv(Dw(kiso, argnum=1), argnum=0)))
    return out


@pytest.mark.parametrize("case", range(4))
def test_one_pair_of_unit_weights_is_bit_identical_to_the_generic_kernel(lp, ctx, case):
    from linpde_gp_amd import _engine
    name, d, k, kk = _descriptor_cases(lp)[case]
    rng = np.random.default_rng(130 + case)
    P0, P1 = _engine.Points(ctx, rng.uniform(-1, 1, (70, d))), _engine.Points(ctx, rng.uniform(-1, 1, (130, d)))
    desc = kk.lower()
    ctx.set_option("asm_fast", 0)               # the generic assemble_kernel, as test_specialised_assembly_is_bit_identical forces it
    try:
        ref = _two_block_matrix(ctx, P0, P1, k.lower())
        ref.assemble(desc, P1, P0, 1, 0)
        ref.assemble(desc, P1, None, 1, 1)
        want = ref.todense("gram")
    finally:
        ctx.set_option("asm_fast", 1)
    got = []
    for _ in range(2):
        M = _two_block_matrix(ctx, P0, P1, k.lower())
        M.assemble_weighted([(desc, 0, 0)], np.ones((1, 130)), np.ones((1, 70)), P1, P0, 1, 0)
        M.assemble_weighted([(desc, 0, 0)], np.ones((1, 130)), None, P1, None, 1, 1)
        got.append(M.todense("gram"))
    assert np.all(np.isfinite(want)) and np.abs(want[70:, :70]).max() > 0
    assert got[0].tobytes() == want.tobytes(), name          # bit for bit, the sign of a zero included
    assert got[0].tobytes() == got[1].tobytes(), name


# ---- entry parity against the oracle ----------------------------------------------------------------------------------------
_KERNEL2 = [(1.0, [("matern", 2.5, 1.0), ("matern", 2.5, 0.7)]), (0.5, [("matern", 3.5, 0.8), ("matern", 3.5, 1.2)])]      # two summands


def _zeros_in_places(X):
    v = np.sin(5 * X[:, 0])
    v[::7] = 0.0                                 # exact zeros
    return v


_OP3 = [((lambda X: -(1 + 0.5 * X[:, 0] * X[:, 1])), {(2, 0): 1.0, (0, 2): 1.0}), ((lambda X: X[:, 1] - 0.2), {(1, 0): 1.0}),
        (_zeros_in_places, {(0, 0): 1.0})]
_OP2 = [((lambda X: np.cos(3 * X[:, 1])), {(0, 1): 1.0, (0, 0): 0.5}), ((lambda X: X[:, 0] ** 3 - 0.1), {(2, 0): 1.0})]


def _entry_bound(env, absw, npairs):
    return ENTRY_RTOL * absw + npairs * EPS * env


def _pairs(lp, kernel, op0, op1):
    from linpde_gp_amd.randprocs import _gaussian_process as gps
    base = vr.lp_kernel(lp, kernel)
    return [(gps._lowered(base, Da, Db), a, b) for a, (_, Da) in enumerate(op0) for b, (_, Db) in enumerate(op1)]


def test_weighted_blocks_against_the_oracle_entry_by_entry(lp, ctx):
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(2)
    X0, X1, Xt = rng.uniform(-1, 1, (70, 2)), rng.uniform(-1, 1, (130, 2)), rng.uniform(-1, 1, (33, 2))
    P0, P1, Pt = _engine.Points(ctx, X0), _engine.Points(ctx, X1), _engine.Points(ctx, Xt)
    ident = [(None, ocf.identity(2))]
    k00 = _pairs(lp, _KERNEL2, ident, ident)[0][0]
    W3, W2 = vr.weights(_OP3, X1), vr.weights(_OP2, X0)
    assert (W3 < 0).any() and (W3 > 0).any() and (W3[2] == 0.0).sum() >= 10 and (W2 < 0).any() and (W2 > 0).any()
    M = _two_block_matrix(ctx, P0, P1, k00)
    M.assemble_weighted(_pairs(lp, _KERNEL2, _OP3, _OP2), W3, W2, P1, P0, 1, 0)            # 130 x 70, A0 = 3, A1 = 2: 6 pairs
    M.assemble_weighted(_pairs(lp, _KERNEL2, _OP3, _OP3), W3, None, P1, None, 1, 1)        # 130 x 130, 9 pairs, 6 distinct shapes
    G = M.todense("gram")
    for what, got, (ref, env, absw), npairs in [("130 x 70", G[70:, :70], vr.block(_KERNEL2, _OP3, _OP2, X1, X0), 6),
                                                ("130 diagonal", G[70:, 70:], vr.block(_KERNEL2, _OP3, _OP3, X1, X1), 9)]:
        ratio = np.abs(got - ref) / _entry_bound(env, absw, npairs)
        print(f"{what}: worst entry at {ratio.max():.3f} of its bound; max |ref| {np.abs(ref).max():.3e}")
        assert ratio.max() <= 1.0, what
    assert np.array_equal(G, G.T)
    # the cross kernel: rows of block 1 of K_Xx, test side unweighted
    rhs = _engine.Rhs(ctx, M, 33)
    rhs.cross_assemble(k00, P0, Pt, 0)
    rhs.cross_assemble_weighted(_pairs(lp, _KERNEL2, _OP3, ident), W3, P1, Pt, 1)
    K = rhs.to_host()
    ref, env, absw = vr.block(_KERNEL2, _OP3, ident, X1, Xt)
    ratio = np.abs(K[70:] - ref) / _entry_bound(env, absw, 3)
    print(f"130 x 33 cross: worst entry at {ratio.max():.3f} of its bound")
    assert ratio.max() <= 1.0
    ref0 = ocf.LkL(_KERNEL2, ocf.identity(2), ocf.identity(2), X0, Xt)
    assert np.abs(K[:70] - ref0).max() <= ENTRY_RTOL * np.abs(ref0).max()


# ---- posterior parity ------------------------------------------------------------------------------------------------------
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_problems_with_the_module():
    yield
    _cache.clear()                               # (device handles must not outlive the library at interpreter exit)


def _problem(lp, name):
    """(posterior through the public interface, dense reference, test points as passed, as (M, d)); built once per session."""
    if name not in _cache:
        if name.startswith("1d"):
            kernel, obs, Xt = vr.problem_1d("boundary first" if name == "1d boundary first" else "pde first")
            u, xt = vr.condition(lp, kernel, obs, scalar_input=True), Xt[:, 0]
        elif name == "2d grid":
            kernel, obs, Xt, g = vr.problem_2d()
            grid = lp.domains.TensorProductGrid(g, g)
            u, xt = vr.condition(lp, kernel, obs, X_as=[None] * 4 + [grid]), Xt
        else:
            kernel, obs, Xt = vr.problem_two_variable_blocks()
            u, xt = vr.condition(lp, kernel, obs), Xt
        _cache[name] = (u, vr.Reference(kernel, obs), xt, Xt)
    return _cache[name]


def test_a_tensor_grid_block_goes_entry_wise(lp, ctx, kronecker_everywhere):
    """The 15 x 15 `TensorProductGrid` block of the 2-D problem is not a Kronecker product: with grids of ANY size allowed onto the
    Kronecker path, its row is still assembled by the per-entry kernels alone (the problem is built here, not taken from the cache)."""
    kernel, obs, _, g = vr.problem_2d()
    grid = lp.domains.TensorProductGrid(g, g)
    ctx.profile_reset(); ctx.profile_enable(["assemble", "assemble_grid"])
    try:
        u = vr.condition(lp, kernel, obs, X_as=[None] * 4 + [grid])
        prof = ctx.profile_get()
    finally:
        ctx.profile_enable(False)
    assert u._blocks[4].points.grid_factors is not None          # (the plain path would have taken the Kronecker assembly)
    assert u._blocks[4].vterms is not None and len(u._blocks[4].vterms) == 4
    assert prof["assemble"]["launches"] >= 5 and prof["assemble_grid"]["launches"] == 0, prof


@pytest.mark.parametrize("name", ["1d boundary first", "1d pde first", "2d grid", "two variable blocks"])
def test_posterior_against_the_dense_reference(lp, ctx, name):
    u, R, xt, Xt = _problem(lp, name)
    mean, var = u.predict(xt)
    rm, rv = R.predict(Xt)
    ma, va = posterior_tolerances(rm, rv)
    em, ev = np.abs(mean - rm).max(), np.abs(var - rv).max()
    w = u.representer_weights
    ew, wa = np.abs(w - R.w).max(), POSTERIOR_RTOL * np.abs(R.w).max()
    print(f"{name}: n={R.r.size}  mean err {em:.3e} / {ma:.3e}   var err {ev:.3e} / {va:.3e}   weights err {ew:.3e} / {wa:.3e}")
    assert em <= ma and ev <= va and ew <= wa
    # the other read-outs of the same factor: mean / var / std alone, the covariance matrix and operator
    np.testing.assert_allclose(u.mean(xt), rm, rtol=0, atol=ma)
    np.testing.assert_allclose(u.std(xt) ** 2, rv, rtol=0, atol=va)
    K = R.cross(Xt[:9])
    d = Xt.shape[1]
    cov = ocf.LkL(R.kernel, ocf.identity(d), ocf.identity(d), Xt[:9], Xt[:9]) - K @ scipy.linalg.cho_solve((R.chol, True), K.T)
    np.testing.assert_allclose(u.cov.matrix(xt[:9]), cov, rtol=0, atol=va)
    np.testing.assert_allclose(u.cov.linop(xt[:9]).todense(), cov, rtol=0, atol=va)


def test_two_variable_blocks_factor_a_doubly_weighted_block(lp):
    u, R, _, _ = _problem(lp, "two variable blocks")
    assert [len(ob.vterms) for ob in u._blocks] == [2, 3] and [ob.points.n for ob in u._blocks] == [70, 130]
    Lf = u.gram.cholesky()
    np.testing.assert_allclose(Lf @ Lf.T, R.G, rtol=0, atol=1e-12 * np.abs(R.G).max())


def test_constant_weights_match_the_constant_coefficient_path(lp, ctx):
    from linpde_gp_amd import _engine
    from linpde_gp_amd.linfuncops import Identity, diffops
    from linpde_gp_amd.randprocs import _gaussian_process as gps
    fn, VCO = lp.functions, diffops.VariableCoefficientOperator
    rng = np.random.default_rng(4)
    Xb, Xc, Xt = rng.uniform(-1, 1, (70, 2)), rng.uniform(-1, 1, (130, 2)), rng.uniform(-1, 1, (33, 2))
    k = vr.lp_kernel(lp, [(1.0, [("matern", 2.5, 1.0), ("matern", 2.5, 0.8)])])
    Lap, Dx = diffops.Laplacian((2,)), diffops.DirectionalDerivative([1.0, 0.0])
    Lv = VCO((2,), [(fn.Constant((2,), -0.7), Lap), (fn.Constant((2,), -1.3), Dx), (None, 2.0 * Identity((2,)))])
    Lc = -0.7 * Lap + (-1.3) * Dx + 2.0 * Identity((2,))
    Yb, Yc = np.sin(Xb[:, 0]), np.cos(Xc[:, 1])
    post = []
    for L in (Lv, Lc):
        u = lp.GaussianProcess(fn.Zero((2,)), k).condition_on_observations(Yb, Xb, b=lp.randvars.Normal(np.zeros(70), np.full(70, 1e-4)))
        u = u.condition_on_observations(Yc, Xc, L=L, b=lp.randvars.Normal(np.zeros(130), np.full(130, 1e-4)))
        post.append((*u.predict(Xt), u.representer_weights))
    assert post[0][0].tobytes() != b"" and u._blocks[1].vterms is None
    for got, want, what in zip(post[0], post[1], ("mean", "var", "weights")):
        err, tol = np.abs(got - want).max(), POSTERIOR_RTOL * np.abs(want).max()
        print(f"constant weights, {what}: err {err:.3e} / {tol:.3e}")
        assert err <= tol
    # one term of weight exactly 1: the same Gram matrix bit for bit, through the block-row assembly of the conditioning
    c = {(2, 0): -1.0, (0, 2): -1.0}
    ident = {(0, 0): 1.0}
    Pb, Pc = _engine.Points(ctx, Xb), _engine.Points(ctx, Xc)
    grams = []
    for coeffs in (c, gps._VariableCoeffs(np.ones((1, 130)), [c])):
        blocks = [gps._ObservationBlock(Yb, None, None, Xb, ident, Pb, None), gps._ObservationBlock(Yc, None, None, Xc, coeffs, Pc, None)]
        M = _engine.GramMatrix(ctx)
        for i, bi in enumerate(blocks):
            M.add_block(bi.points.n)
            for j, bj in enumerate(blocks[:i + 1]):
                gps._assemble_block(M, k, i, j, bi, bj)
        grams.append(M.todense("gram"))
    assert np.abs(grams[0][70:, 70:]).max() > 1 and np.array_equal(grams[0], grams[1])


def test_downstream_of_the_factor(lp):
    u, R, xt, _ = _problem(lp, "1d boundary first")
    n = R.r.size
    sign, logdet = np.linalg.slogdet(R.G)
    quad = float(R.r @ R.w)
    want = -0.5 * quad - 0.5 * logdet - 0.5 * n * np.log(2 * np.pi)
    lam = np.linalg.eigvalsh(R.G)
    slack = 2.0 * n * np.sqrt(3.0 * n + 1.0) * 2.0 ** -53 * lam[-1] * float(R.w @ R.w)        # tests/test_gpu_evidence.py: _quad_slack
    got = u.log_marginal_likelihood()
    print(f"lml {got:.15e} (ref {want:.15e}), slack {0.5 * slack + 0.5e-9 * abs(logdet):.3e}; logdet {u.gram.logabsdet():.15e} (ref {logdet:.15e})")
    assert sign == 1.0 and abs(got - want) <= 0.5 * slack + 0.5e-9 * abs(logdet)
    assert abs(u.gram.logabsdet() - logdet) <= 1e-9 * abs(logdet)
    Ginv = scipy.linalg.cho_solve((R.chol, True), np.eye(n))
    dd = np.diag(Ginv)
    logp = 0.5 * np.log(dd) - 0.5 * R.w ** 2 / dd - 0.5 * np.log(2 * np.pi)
    loo = u.leave_one_out()
    print(f"loo total {loo.total:.12e} (ref {np.sum(logp):.12e})")
    assert abs(loo.total - np.sum(logp)) <= POSTERIOR_RTOL * np.max(np.abs(logp)) * logp.size
    draws = u.sample(np.random.default_rng(0), xt, size=4)
    assert draws.shape == (4, 33) and np.all(np.isfinite(draws))
    # trace and products of the Gram operator re-evaluate the weighted blocks
    assert abs(u.gram.trace() - np.trace(R.G)) <= 1e-12 * np.trace(R.G)
    V = np.random.default_rng(1).standard_normal((n, 2))
    np.testing.assert_allclose(u.gram @ V, R.G @ V, rtol=0, atol=1e-11 * np.abs(R.G).max() * n)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_not_implemented_cases_name_the_feature(lp, ctx, monkeypatch):
    from linpde_gp_amd import _spawn, config
    from linpde_gp_amd.linfuncops import diffops
    u, _, xt, _ = _problem(lp, "1d boundary first")
    L = diffops.VariableCoefficientOperator((), [(lp.functions.Polynomial([1.0, 0.5]), diffops.Derivative(1))])
    X, Y = np.linspace(-0.5, 0.5, 5), np.zeros(5)
    nblocks = u._state.mat.num_blocks
    with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
        u.log_marginal_likelihood_gradient()
    with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
        L(u)
    with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
        L.to_linfunctl(X)(u)
    prior = u.prior
    monkeypatch.setattr(config, "matrix_free", True)
    with pytest.raises(NotImplementedError, match="matrix-free"):
        prior.condition_on_observations(Y, X, L=L)
    monkeypatch.setattr(config, "matrix_free", False)
    monkeypatch.setattr(config, "matrix_free_above", 100)
    with pytest.raises(NotImplementedError, match="matrix-free"):
        u.condition_on_observations(Y, X)                      # a chain with a variable block outgrowing the dense path
    monkeypatch.setattr(config, "matrix_free_above", 0)
    monkeypatch.setattr(_spawn, "_active", object())
    with pytest.raises(NotImplementedError, match="lp.spawn"):
        prior.condition_on_observations(Y, X, L=L)
    monkeypatch.setattr(_spawn, "_active", None)
    monkeypatch.setattr(ctx, "distributed", True)              # what a context that joined a multi-GPU job says
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        prior.condition_on_observations(Y, X, L=L)
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        u.condition_on_observations(Y, X, L=L)
    monkeypatch.setattr(ctx, "distributed", False)
    assert u._state.mat.num_blocks == nblocks
    u2 = u.condition_on_observations(Y, X, L=L, b=lp.randvars.Normal(np.zeros(5), np.full(5, 1e-2)))       # and the path itself still works
    assert np.all(np.isfinite(u2.mean(xt)))


def test_c_abi_refusals_leave_the_matrix_untouched(lp, ctx):
    from linpde_gp_amd import _engine, _lib
    lib = _lib.lib
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(6)
    X0, X1 = rng.uniform(-1, 1, (70, 2)), rng.uniform(-1, 1, (130, 2))
    P0, P1, P3 = _engine.Points(ctx, X0), _engine.Points(ctx, X1), _engine.Points(ctx, rng.uniform(-1, 1, (130, 3)))
    k = cf.TensorProduct(cf.Matern((), nu=2.5), cf.Matern((), nu=2.5))
    k3 = cf.TensorProduct(cf.Matern((), nu=2.5), cf.Matern((), nu=2.5), cf.Matern((), nu=2.5))
    kd, kd3 = _engine.lowered_array(k.lower()), _engine.lowered_array(k3.lower())
    M = _engine.GramMatrix(ctx)
    M.add_block(70); M.add_block(130)
    M.assemble(kd, P0, None, 0, 0); M.assemble(kd, P1, P0, 1, 0); M.assemble(kd, P1, None, 1, 1)
    M.add_diag(0, None, 1e-3); M.add_diag(1, None, 1e-3)
    before = M.todense("gram")
    w0, w1 = np.full((2, 130), 2.0), np.full((2, 70), 3.0)

    def call(pairs, a0=w0, A0=2, a1=w1, A1=2, X0_=P1, X1_=P0, bi=1, bj=0, npairs=None):
        arr, keep = _engine._wpair_array(pairs)
        return lib.lpgp_gram_assemble_weighted(ctx._h, arr, len(arr) if npairs is None else npairs, _lib.as_pd(a0) if a0 is not None else None, A0,
                                               _lib.as_pd(a1) if a1 is not None else None, A1, X0_._h, X1_._h if X1_ is not None else None, M._h, bi, bj)

    one = [(kd, 0, 0)]
    bad = {
        "npairs = 0": lambda: call(one, npairs=0),
        "npairs = 17": lambda: call(one * 17),
        "A0 = 0": lambda: call(one, A0=0),
        "A0 = 5": lambda: call(one, A0=5),
        "A1 = 5": lambda: call(one, A1=5),
        "A1 = 0 off the diagonal": lambda: call(one, A1=0),
        "row index out of range": lambda: call([(kd, 2, 0)]),
        "negative column index": lambda: call([(kd, 0, -1)]),
        "null row weights": lambda: call(one, a0=None),
        "null column weights": lambda: call(one, a1=None),
        "column weights on a diagonal block": lambda: call(one, X1_=None, bj=1),
        "asymmetric diagonal list": lambda: call([(kd, 0, 1)], a1=None, X1_=None, bj=1),
        "mixed input dimension": lambda: call([(kd, 0, 0), (kd3, 1, 1)]),
        "points of another dimension": lambda: call(one, X0_=P3),
        "block above the diagonal": lambda: call(one, bi=0, bj=1),
    }
    for what, f in bad.items():
        rc = f()
        msg = lib.lpgp_last_error().decode()
        assert rc != 0 and "lpgp_gram_assemble_weighted" in msg, (what, rc, msg)
        with pytest.raises(_lib.LpgpError):
            _lib.check(rc, what)
        assert M.num_blocks == 2 and M.n == 200, what
    # the cross entry point: b must be 0, the weights must be there
    rhs = _engine.Rhs(ctx, M, 70)
    arr, keep = _engine._wpair_array([(kd, 0, 1)])
    assert lib.lpgp_cross_assemble_weighted(ctx._h, arr, 1, _lib.as_pd(w0), 2, P1._h, P0._h, rhs._h, M._h, 1) != 0
    arr, keep = _engine._wpair_array(one)
    assert lib.lpgp_cross_assemble_weighted(ctx._h, arr, 1, None, 2, P1._h, P0._h, rhs._h, M._h, 1) != 0
    assert lib.lpgp_cross_assemble_weighted(ctx._h, arr, 1, _lib.as_pd(w0), 5, P1._h, P0._h, rhs._h, M._h, 1) != 0
    assert np.array_equal(M.todense("gram"), before)            # nothing was written by any refused call
    # a factored block, and a strict-prefix view
    assert M.potrf() == 0
    factor = M.todense("factor")
    with pytest.raises(_lib.LpgpError, match="already factored"):
        M.assemble_weighted(one, w0, w1, P1, P0, 1, 0)
    M.add_block(130)
    M.assemble(kd, P1, P0, 2, 0); M.assemble(kd, P1, P1, 2, 1); M.assemble(kd, P1, None, 2, 2)
    M.add_diag(2, None, 1e-2)
    assert M.potrf() == 0
    M.set_view(2)
    with pytest.raises(_lib.LpgpError, match="strict prefix"):
        M.assemble_weighted(one, w0, w1, P1, P0, 1, 0)
    assert M.num_blocks == 2 and M.n == 200 and np.array_equal(M.todense("factor"), factor)
    M.set_view(-1)
    # ... and an ordinary conditioning afterwards is what it always was
    Y = np.sin(X0[:, 0])
    b = lp.randvars.Normal(np.zeros(70), np.full(70, 1e-3))
    m1 = lp.GaussianProcess(lp.functions.Zero((2,)), k).condition_on_observations(Y, X0, b=b).mean(X1)
    w = scipy.linalg.cho_solve(scipy.linalg.cho_factor(before[:70, :70]), Y)
    np.testing.assert_allclose(m1, before[70:, :70] @ w, rtol=0, atol=POSTERIOR_RTOL * np.abs(m1).max())


def test_c_abi_refuses_a_context_inside_a_multi_gpu_job(lp, ctx):
    """A second context on the same device joins a job of one rank over the host-staged transport (`lpgp_dist_init_host`): from
    then on it is distributed, and both weighted entry points refuse it before they look at anything else."""
    from linpde_gp_amd import _engine, _lib
    lib = _lib.lib
    cf = lp.randprocs.covfuncs
    ctx2 = _engine.Context(ctx.device)
    try:
        X = np.random.default_rng(8).uniform(-1, 1, (70, 2))
        kd = _engine.lowered_array(cf.TensorProduct(cf.Matern((), nu=2.5), cf.Matern((), nu=2.5)).lower())
        P = _engine.Points(ctx2, X)
        M = _engine.GramMatrix(ctx2)
        M.add_block(70)
        M.assemble(kd, P, None, 0, 0)
        before = M.todense("gram")
        rhs = _engine.Rhs(ctx2, M, 70)
        exchange = _lib.HOST_EXCHANGE_FN(lambda user, op, buf, nbytes, root: 0)
        _lib.check(lib.lpgp_dist_init_host(ctx2._h, 0, 1, exchange, None), "lpgp_dist_init_host")
        with pytest.raises(_lib.LpgpError, match="lpgp_gram_assemble_weighted: single GPU only"):
            M.assemble_weighted([(kd, 0, 0)], np.ones((1, 70)), None, P, None, 0, 0)
        with pytest.raises(_lib.LpgpError, match="lpgp_cross_assemble_weighted: single GPU only"):
            rhs.cross_assemble_weighted([(kd, 0, 0)], np.ones((1, 70)), P, P, 0)
        assert M.num_blocks == 1 and M.n == 70
        del rhs, M, P
    finally:
        ctx2.close()


def test_not_positive_definite_raises_and_the_earlier_posterior_is_intact(lp):
    from linpde_gp_amd.linfuncops import diffops
    u, _, xt, _ = _problem(lp, "1d pde first")
    u.representer_weights                                       # (both predictions below form the mean from the weights)
    u._pred_cache = None
    before = u.predict(xt)
    nblocks, n = u._state.mat.num_blocks, u._state.mat.n
    L = diffops.VariableCoefficientOperator((), [(lp.functions.Polynomial([1.0, 0.5]), diffops.Derivative(1)), (None, diffops.Derivative(0))])
    X = np.repeat(np.linspace(-0.9, 0.9, 35), 2)                # every point twice, no noise: singular
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        u.condition_on_observations(np.zeros(70), X, L=L)
    assert u._state.mat.num_blocks == nblocks and u._state.mat.n == n
    u._pred_cache = None
    after = u.predict(xt)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
