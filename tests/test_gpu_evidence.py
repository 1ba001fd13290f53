"""Model evidence and leave-one-out diagnostics from the resident factor (csrc/evidence.hip): `lpgp_mat_evidence`,
`lpgp_mat_inverse_diag`, `lpgp_mat_loo` through the public interface -- `log_marginal_likelihood()`, `leave_one_out()`,
`gram.inv().diagonal()`, `Normal.logpdf` / `entropy` -- and through the binding, against NumPy on the oracle's Gram matrix
and the closed-form reference of tests/_evidence_reference.py (itself checked in tests/test_evidence_host.py).

Bounds.  log det: the 1e-9 relative bound of `gram.logabsdet()` (test_gpu_parity.py).  Quadratic form q = r^T G^-1 r: both
the device and the LAPACK reference compute r^T (G + dG)^-1 r for a backward error dG of their Cholesky factorisation and
substitution, |dG| <= gamma_(3n+1) |L| |L^T| (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4) with
|| |L| |L^T| ||_2 <= n ||G||_2 (eq. 10.7), and gamma_k ~ sqrt(k) u for rounding errors that do not conspire (Higham & Mary
2019).  To first order |dq| = |w^T dG w| <= ||dG||_2 ||w||^2, w = G^-1 r, ||w||^2 <= ||r||^2 / lambda_min^2, so
    |dq| <= n sqrt(3n + 1) u ||G||_2 ||w||^2 <= n sqrt(3n + 1) u cond_2(G) ||r||^2 / lambda_min
per computation, twice that between two of them.  `_quad_slack` evaluates both forms from the matrix's own spectrum (the
first with the reference's w); the test holds the device to the first, the smaller one.  Everything else: the posterior criterion of conftest.py,
max |delta| <= 1e-8 max |ref|, on noisy problems (cond <= 1e6)."""
import numpy as np
import pytest
import scipy.linalg
import scipy.stats

import _evidence_reference as ref
from conftest import POSTERIOR_RTOL
from oracle import covfuncs as ocf
from oracle import gp as ogp
from oracle import workloads as owl

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lp():
    import linpde_gp_amd
    return linpde_gp_amd


@pytest.fixture(params=["eager", "lazy"])
def mode(lp, request):
    saved = lp.config.lazy_factorization
    lp.config.lazy_factorization = request.param == "lazy"
    yield request.param
    lp.config.lazy_factorization = saved


def _close(got, want, what):
    tol = POSTERIOR_RTOL * float(np.max(np.abs(want)))
    err = float(np.max(np.abs(np.asarray(got) - want)))
    print(f"{what}: max abs err {err:.3e}, bound {tol:.3e}")
    assert err <= tol, f"{what}: max abs err {err:.3e} > {tol:.3e} (1e-8 of max |ref|)"


def _quad_slack(G, r, w):
    lam = np.linalg.eigvalsh(G)
    n = r.size
    c = 2.0 * n * np.sqrt(3.0 * n + 1.0) * U
    slack, loose = c * lam[-1] * float(w @ w), c * (lam[-1] / lam[0]) * float(r @ r) / lam[0]
    assert slack <= loose * (1 + 1e-6)
    return slack, lam[-1] / lam[0]


# ---- the problems: (posterior built through the public interface, oracle Gram matrix, residual, observations) ----------------
def _noisy_1d(lp, n=300, seed=3, noise=1e-2, want_ref=True):
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(-1, 1, n))[:, None]
    Y = 0.5 + np.sin(3 * X[:, 0]) + np.sqrt(noise) * rng.standard_normal(n)
    prior = lp.GaussianProcess(lp.functions.Constant((1,), 0.5), 1.3 * cf.Matern((1,), nu=2.5, lengthscales=0.5))
    u = prior.condition_on_observations(Y, X, b=lp.randvars.Normal(np.zeros(n), np.full(n, noise)))
    blocks = [ogp.ObsBlock(X, ocf.identity(1), Y, None, noise)]
    return u, ogp.gram(ref.Problem40.kernel, blocks) if want_ref else None, ogp.residual(blocks, 0.5), Y


def _chain_1d(lp, sizes=(150, 70, 200), seed=11):
    """Value observations appended block by block on ragged sizes; returns every posterior of the chain with its reference."""
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(seed)
    prior = lp.GaussianProcess(lp.functions.Zero((1,)), 1.3 * cf.Matern((1,), nu=2.5, lengthscales=0.5))
    u, blocks, out = prior, [], []
    for k, n in enumerate(sizes):
        X = rng.uniform(-1, 1, (n, 1))
        noise = rng.uniform(1e-2, 2e-2, n)
        Y = np.sin(3 * X[:, 0]) + np.sqrt(noise) * rng.standard_normal(n)
        u = u.condition_on_observations(Y, X, b=lp.randvars.Normal(np.zeros(n), noise))
        blocks.append(ogp.ObsBlock(X, ocf.identity(1), Y, None, np.diag(noise)))
        out.append((u, ogp.gram(ref.Problem40.kernel, blocks), ogp.residual(blocks), np.concatenate([b.Y for b in blocks])))
    return out


def _workload(lp, wl):
    from linpde_gp_amd import problems, randvars
    u = problems.build_prior(wl)
    for o in wl.observations:
        X, Y = o.X_as_given()
        b = None if o.noise_var is None else randvars.Normal(np.zeros(Y.shape), np.full(o.X.shape[0], o.noise_var))
        u = u.condition_on_observations(Y, X=X, L=problems.operator_of(o.op, wl.d), b=b)
    blocks = owl.blocks_of(wl)
    return u, ogp.gram(wl.kernel, blocks), ogp.residual(blocks), np.concatenate([o.Y for o in wl.observations])


def _case(lp, name):
    from linpde_gp_amd import problems
    if name == "noisy_1d":
        return _noisy_1d(lp)
    if name == "c1":
        return _workload(lp, problems.poisson_1d(512, n_bdry_repeats=16, noise_var=1e-4, m=256))
    if name == "poisson2d_ragged_chain":       # four boundary blocks of 23 rows, then 19 x 19 collocation rows: five appends, none a multiple of the tile
        return _workload(lp, problems.poisson_2d(n_side=19, n_bdry=23, m_side=4))
    chain = _chain_1d(lp)                        # "earlier_view": the FIRST posterior, asked after two more blocks were appended
    return chain[0]


_results = {}


@pytest.mark.parametrize("name", ["noisy_1d", "c1", "poisson2d_ragged_chain", "earlier_view"])
def test_evidence_against_the_oracle_gram(lp, mode, name):
    u, G, r, _ = _case(lp, name)
    sign, logdet = np.linalg.slogdet(G)
    w = scipy.linalg.cho_solve(scipy.linalg.cho_factor(G, lower=True), r)
    quad = float(r @ w)
    want = -0.5 * quad - 0.5 * logdet - 0.5 * r.size * np.log(2 * np.pi)
    got = u.log_marginal_likelihood()
    q_dev, ld_dev = u._state.mat.evidence(u._residual())          # the two terms apart (the view is this posterior's: just used)
    slack, cond = _quad_slack(G, r, w)
    print(f"{name} [{mode}]: n={r.size} cond2={cond:.3e}  logdet {ld_dev:.15e} (ref {logdet:.15e}, rel {abs(ld_dev - logdet) / abs(logdet):.2e})  "
          f"quad {q_dev:.15e} (ref {quad:.15e}, err {abs(q_dev - quad):.3e}, slack {slack:.3e})  lml {got:.15e} (ref {want:.15e})")
    assert sign == 1.0 and abs(ld_dev - logdet) <= 1e-9 * abs(logdet)
    assert abs(q_dev - quad) <= slack
    assert got == -0.5 * q_dev - 0.5 * ld_dev - 0.5 * r.size * np.log(2 * np.pi)
    assert abs(got - want) <= 0.5 * slack + 0.5e-9 * abs(logdet)
    _results[(name, mode)] = got
    other = _results.get((name, "lazy" if mode == "eager" else "eager"))
    if other is not None:
        print(f"{name}: eager / lazy differ by {abs(got - other) / abs(got):.2e} (relative)")
        assert abs(got - other) <= 1e-12 * abs(got)


def test_bit_reproducible(lp):
    u, G, r, Y = _noisy_1d(lp, n=700, seed=5)
    u._check_current()
    mat = u._state.mat
    a, b = mat.evidence(r), mat.evidence(r)
    assert np.array([a]).tobytes() == np.array([b]).tobytes()
    la, lb = mat.loo(r, Y), mat.loo(r, Y)
    for x, y in zip(la, lb):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    ctx = mat.ctx
    ctx.set_option("trsv_resident", 0)          # the per-tile form of the single-vector solve: other kernels, the same contract
    try:
        c, d = mat.evidence(r), mat.evidence(r)
    finally:
        ctx.set_option("trsv_resident", 1)
    assert np.array([c]).tobytes() == np.array([d]).tobytes()
    assert abs(c[0] - a[0]) <= 1e-10 * abs(a[0]) and c[1] == a[1]


@pytest.fixture
def panel(lp):
    from linpde_gp_amd import _engine
    ctx = _engine.default_context()
    saved = ctx.get_option("inverse_diag_panel")
    yield lambda v: ctx.set_option("inverse_diag_panel", v)
    ctx.set_option("inverse_diag_panel", saved)


@pytest.mark.parametrize("name,width", [("one_tile", 4096), ("several_panels", 256), ("several_panels", 128), ("ragged_chain", 256)])
def test_inverse_diag(lp, panel, name, width):
    """n = 100: one tile.  n = 700 (768 padded) with panels of 256 and of 128 columns: three and six panels, every one after
    the first solved against a trailing sub-factor.  Blocks of 150 + 70 + 200 rows (256 + 128 + 256 padded) with panels of
    256: panel boundaries on and off block boundaries, padding rows inside every panel."""
    assert lp.randprocs  # (the package is loaded)
    if name == "ragged_chain":
        u, G, r, _ = _chain_1d(lp)[-1]
    else:
        u, G, r, _ = _noisy_1d(lp, n=100 if name == "one_tile" else 700, seed=7)
    assert np.linalg.cond(G) <= 1e6
    panel(width)
    assert u._state.ctx.get_option("inverse_diag_panel") == width
    want = np.diag(np.linalg.inv(G))
    got = u.gram.inv().diagonal()
    assert got.shape == want.shape
    _close(got, want, f"diag(G^-1) {name}, panels of {width}")
    _close(got, np.diag(u.gram.inv().todense()), f"diagonal() vs diag(todense()) {name}")
    panel(4096)
    full = u.gram.inv().diagonal()              # the panel width changes the schedule of the solve, not what is computed
    _close(full, want, f"diag(G^-1) {name}, one panel")


def test_inverse_diag_panel_option(lp, panel):
    for bad in (0, 100, 4224, -128):
        with pytest.raises(Exception, match="inverse_diag_panel must be a multiple of 128"):
            panel(bad)
    panel(384)


def test_loo_against_the_closed_forms(lp, mode, panel):
    panel(256)
    for u, G, r, Y in (_noisy_1d(lp, n=300), _chain_1d(lp)[-1], _chain_1d(lp)[0]):
        mean, var, logp = ref.loo(G, r, Y)
        got = u.leave_one_out()
        _close(got.mean, mean, "LOO mean")
        _close(got.var, var, "LOO variance")
        _close(got.std, np.sqrt(var), "LOO std")
        _close(got.log_predictive_density, logp, "LOO log density")
        assert abs(got.total - np.sum(logp)) <= POSTERIOR_RTOL * np.max(np.abs(logp)) * logp.size
        assert abs(got.total - np.sum(got.log_predictive_density)) <= 1e-13 * np.sum(np.abs(logp))


def test_loo_against_brute_force_reconditioning(lp):
    """The 40-point problem of the host test: 40 conditionings through the public interface that each leave one point out,
    `predict` at that point, plus the point's own noise."""
    cf = lp.randprocs.covfuncs
    p = ref.Problem40()
    prior = lp.GaussianProcess(lp.functions.Constant((1,), p.mean_const), 1.3 * cf.Matern((1,), nu=2.5, lengthscales=0.5))
    u = prior.condition_on_observations(p.Y, p.X, b=lp.randvars.Normal(p.noise_mean, p.noise_var))
    got = u.leave_one_out()
    mean, var = np.empty(40), np.empty(40)
    for i in range(40):
        keep = np.arange(40) != i
        ui = prior.condition_on_observations(p.Y[keep], p.X[keep], b=lp.randvars.Normal(p.noise_mean[keep], p.noise_var[keep]))
        m, v = ui.predict(p.X[i:i + 1])
        mean[i], var[i] = m[0] + p.noise_mean[i], v[0] + p.noise_var[i]
    logp = -0.5 * (p.Y - mean) ** 2 / var - 0.5 * np.log(var) - 0.5 * np.log(2 * np.pi)
    _close(got.mean, mean, "LOO mean vs re-conditioning")
    _close(got.var, var, "LOO variance vs re-conditioning")
    _close(got.log_predictive_density, logp, "LOO log density vs re-conditioning")
    rm, rv, rl = ref.loo(p.G, p.r, p.Y)
    _close(got.mean, rm, "LOO mean vs closed form")
    _close(got.var, rv, "LOO variance vs closed form")
    _close(got.log_predictive_density, rl, "LOO log density vs closed form")
    assert abs(u.log_marginal_likelihood() - ref.evidence(p.G, p.r)[2]) <= 1e-9 * abs(ref.evidence(p.G, p.r)[2])


def test_normal_logpdf_and_entropy_dense(lp):
    rng = np.random.default_rng(8)
    n = 200
    A = rng.standard_normal((n, n))
    cov = A @ A.T / n + 0.1 * np.eye(n)
    mean = rng.standard_normal(n)
    N = lp.randvars.Normal(mean, cov)
    sp = scipy.stats.multivariate_normal(mean, cov)
    x = mean + rng.standard_normal((3, n))
    got = N.logpdf(x)
    assert got.shape == (3,)
    np.testing.assert_allclose(got, sp.logpdf(x), rtol=1e-10)
    np.testing.assert_allclose(N.logpdf(x[1]), sp.logpdf(x[1]), rtol=1e-10)
    np.testing.assert_allclose(N.entropy, sp.entropy(), rtol=1e-10)
    # a (10, 13)-shaped variable: the covariance acts on the C-order flattening
    N2 = lp.randvars.Normal(mean[:130].reshape(10, 13), cov[:130, :130])
    sp2 = scipy.stats.multivariate_normal(mean[:130], cov[:130, :130])
    np.testing.assert_allclose(N2.logpdf(x[:, :130].reshape(3, 10, 13)), sp2.logpdf(x[:, :130]), rtol=1e-10)


def test_error_paths(lp):
    from linpde_gp_amd import _engine, _lib, _spawn
    cf = lp.randprocs.covfuncs
    ctx = _engine.default_context()
    # an assembled matrix that was never factored
    k = cf.ExpQuad((1,), lengthscales=1.0)
    S = _engine.GramMatrix(ctx, 64)
    S.add_block(50)
    S.assemble(k.lower(), _engine.Points(ctx, np.linspace(-1, 1, 50)[:, None]), None, 0, 0)
    for call in (lambda: S.evidence(np.zeros(50)), S.inverse_diag, lambda: S.loo(np.zeros(50), np.zeros(50))):
        with pytest.raises(_lib.LpgpError, match=r"matrix is not \(fully\) factored"):
            call()
    with pytest.raises(ValueError):
        S.evidence(np.zeros(49))
    # a lazy factorisation that fails: reported at the first use, as `LinAlgError`, and again on every later use
    prior = lp.GaussianProcess(lp.functions.Zero((1,)), k)
    saved = lp.config.lazy_factorization
    lp.config.lazy_factorization = True
    try:
        X = np.array([[0.0], [0.0], [0.5]])
        bad = prior.condition_on_observations(np.zeros(3), X, b=lp.randvars.Normal(np.zeros(3), -1e-3 * np.eye(3)))
        for _ in range(2):
            with pytest.raises(np.linalg.LinAlgError):
                bad.log_marginal_likelihood()
            with pytest.raises(np.linalg.LinAlgError):
                bad.leave_one_out()
            with pytest.raises(np.linalg.LinAlgError):
                bad.gram.inv().diagonal()
    finally:
        lp.config.lazy_factorization = saved
    # a matrix-free posterior
    X, Y = np.linspace(-1, 1, 20)[:, None], np.zeros(20)
    saved = lp.config.matrix_free
    lp.config.matrix_free = True
    try:
        mf = prior.condition_on_observations(Y, X, b=lp.randvars.Normal(np.zeros(20), 1e-2 * np.eye(20)))
    finally:
        lp.config.matrix_free = saved
    with pytest.raises(NotImplementedError):
        mf.log_marginal_likelihood()
    with pytest.raises(NotImplementedError):
        mf.leave_one_out()
    # spawn proxy (no worker group is started: the proxy refuses before it would talk to one)
    proxy = _spawn.RemoteConditionalGaussianProcess.__new__(_spawn.RemoteConditionalGaussianProcess)
    with pytest.raises(NotImplementedError):
        proxy.log_marginal_likelihood()
    with pytest.raises(NotImplementedError):
        proxy.leave_one_out()
    # nothing observed: the empty product
    empty = prior.condition_on_observations(np.zeros(0), np.zeros((0, 1)))
    assert empty.log_marginal_likelihood() == 0.0 and empty.leave_one_out().mean.shape == (0,)


def test_loo_moves_nothing_of_size_n_squared(lp):
    """`lpgp_mat_loo` at n = 4 096: the library's own count of the bytes it copies -- up: residual, observations and the
    row map (2.5 n doubles); down: mean, variance, log density and their sum (3 n + 1 doubles).  The n x n identity and the
    n x n inverse of the host route would be 2 x 134 MB."""
    n = 4096
    u, _, _, _ = _noisy_1d(lp, n=n, seed=9, want_ref=False)
    ctx = u._state.ctx
    h0, d0 = ctx.get_option("evidence_h2d_bytes"), ctx.get_option("evidence_d2h_bytes")
    got = u.leave_one_out()
    up, down = ctx.get_option("evidence_h2d_bytes") - h0, ctx.get_option("evidence_d2h_bytes") - d0
    print(f"lpgp_mat_loo n={n}: {up} bytes up, {down} bytes down")
    assert down == (3 * n + 1) * 8 and up == (2 * n + n // 2) * 8
    assert np.all(np.isfinite(got.mean)) and np.all(got.var > 0) and np.isfinite(got.total)
    d0 = ctx.get_option("evidence_d2h_bytes")
    u.log_marginal_likelihood()
    assert ctx.get_option("evidence_d2h_bytes") - d0 == 16
    d0 = ctx.get_option("evidence_d2h_bytes")
    u.gram.inv().diagonal()
    assert ctx.get_option("evidence_d2h_bytes") - d0 == n * 8
