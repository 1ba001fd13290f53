"""Observations through a matrix, `A @ L`, on the device: the fused stencil kernel (`assemble_mixed_kernel`, `lpgp_gram_assemble_mixed`,
`lpgp_cross_assemble_mixed`) bit for bit against the generic kernel where the two must agree, entry by entry against the dense
reference `A0 @ K @ A1.T` (tests/_mixed_reference.py) everywhere else, and the posteriors, the quantities downstream of the factor
and the read-out through the public interface.

Entry bound: ENTRY_RTOL * absw + (S0 * S1) * EPS * env -- the unweighted bound of tests/test_gpu_kernels.py on every kernel
value, scaled by the stencils' absolute weights, plus one rounding per term of the fma chain of S0 * S1 terms on the envelope
|A0| |K| |A1|^T.  Sizes 130 and 70 cross the 64-row tile and the 128-row storage tile."""
import numpy as np
import pytest
import scipy.linalg

import _mixed_reference as mr
from _varcoef_reference import lp_kernel
from conftest import POSTERIOR_RTOL, posterior_tolerances

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


def _kernel(d):
    return [(1.7, [("matern", 2.5, 0.6 + 0.3 * j) for j in range(d)])]


def _lap(d):
    return {tuple(2 if i == j else 0 for i in range(d)): -1.0 for j in range(d)}


def _desc(lp, kernel, D0, D1):
    from linpde_gp_amd.randprocs import _gaussian_process as gps
    return gps._lowered(lp_kernel(lp, kernel), D0, D1)


def _table(rng, q, S, npts, ragged=True):
    """A stencil table of q rows: counts 1 .. S in turn (`ragged`), indices shared between rows, negative weights and exact zero
    weights, the padding rule for the short rows."""
    idx = rng.integers(0, npts, (q, S)).astype(np.int32)
    w = rng.normal(size=(q, S))
    w[rng.uniform(size=(q, S)) < 0.1] = 0.0
    idx[1::5, 0] = idx[0, 0]                     # points shared between rows
    if ragged:
        for r in range(q):
            n = 1 + r % S
            w[r, n:] = 0.0
            idx[r, n:] = idx[r, 0]
    return idx, w


def _identity_table(n):
    return np.arange(n, dtype=np.int32)[:, None].copy(), np.ones((n, 1))


def _two_blocks(ctx, n0, n1):
    from linpde_gp_amd import _engine
    M = _engine.GramMatrix(ctx)
    M.add_block(n0)
    M.add_block(n1)
    return M


def _generic(ctx, f):
    ctx.set_option("asm_fast", 0)                # the generic assemble_kernel, as test_specialised_assembly_is_bit_identical forces it
    try:
        return f()
    finally:
        ctx.set_option("asm_fast", 1)


# ---- bit identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3])
def test_identity_stencils_are_bit_identical_to_the_generic_kernel(lp, ctx, d):
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(130 + d)
    X0, X1, Xt = rng.uniform(-1, 1, (70, d)), rng.uniform(-1, 1, (130, d)), rng.uniform(-1, 1, (33, d))
    X1[5] = X1[4]                                # coinciding points: entries whose odd terms are signed zeros
    P0, P1, Pt = _engine.Points(ctx, X0), _engine.Points(ctx, X1), _engine.Points(ctx, Xt)
    desc = _desc(lp, _kernel(d), _lap(d), _lap(d))
    dcross = _desc(lp, _kernel(d), _lap(d), {(0,) * d: 1.0})

    def plain():
        M = _two_blocks(ctx, 70, 130)
        M.assemble(desc, P1, P0, 1, 0)
        M.assemble(desc, P1, None, 1, 1)
        rhs = _engine.Rhs(ctx, M, 33)
        rhs.cross_assemble(dcross, P1, Pt, 1)
        return M.todense("gram")[70:], rhs.to_host()[70:]
    want, want_cross = _generic(ctx, plain)
    I0, I1 = _engine.Mix(ctx, *_identity_table(70), 70), _engine.Mix(ctx, *_identity_table(130), 130)
    got = []
    for t0, t1 in ((I1, I0), (None, None), (I1, I0)):
        M = _two_blocks(ctx, 70, 130)
        M.assemble_mixed(desc, P1, t0, P0, t1, 1, 0)
        M.assemble_mixed(desc, P1, t0, None, None, 1, 1)
        rhs = _engine.Rhs(ctx, M, 33)
        rhs.cross_assemble_mixed(dcross, P1, t0, Pt, 1)
        got.append((M.todense("gram")[70:], rhs.to_host()[70:]))
    assert np.all(np.isfinite(want)) and np.abs(want[:, :70]).max() > 0 and np.abs(want_cross).max() > 0
    for G, Kx in got:
        assert G.tobytes() == want.tobytes()     # the 130 x 70 block and the 130-row diagonal block, the sign of a zero included
        assert Kx.tobytes() == want_cross.tobytes()
    # a permutation as index: the permuted block, bit for bit
    p0, p1 = rng.permutation(70).astype(np.int32), rng.permutation(130).astype(np.int32)
    T0, T1 = _engine.Mix(ctx, p0[:, None].copy(), np.ones((70, 1)), 70), _engine.Mix(ctx, p1[:, None].copy(), np.ones((130, 1)), 130)
    M = _two_blocks(ctx, 70, 130)
    M.assemble_mixed(desc, P1, T1, P0, T0, 1, 0)
    rhs = _engine.Rhs(ctx, M, 33)
    rhs.cross_assemble_mixed(dcross, P1, T1, Pt, 1)
    assert M.todense("gram")[70:, :70].tobytes() == np.ascontiguousarray(want[p1][:, p0]).tobytes()
    assert rhs.to_host()[70:].tobytes() == np.ascontiguousarray(want_cross[p1]).tobytes()


# ---- entry by entry against the reference -------------------------------------------------------------------------------------
def _hold(what, got, ref, env, absw, S0, S1):
    bound = ENTRY_RTOL * absw + (S0 * S1) * EPS * env
    err = np.abs(got - ref)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f}   (max |ref| {np.abs(ref).max():.3e}, {int(np.sum(bound == 0))} entries of rows without weight)")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), what       # (a row of zero weights alone: bound 0, the entry exactly 0)


def test_both_sides_mixed_and_one_side_plain_against_the_reference(lp, ctx):
    """(a) 130 x 70, S0 = 9, S1 = 4, d = 2, ragged rows with counts 1 .. S, shared points, negative and exact zero weights;
    (c) one side plain, each way round; (e) the 130 x 33 cross block; and the same bits on a second call."""
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(94)
    d, kernel, D = 2, _kernel(2), _lap(2)
    X0, X1, Xt = rng.uniform(-1, 1, (50, d)), rng.uniform(-1, 1, (300, d)), rng.uniform(-1, 1, (33, d))
    P0, P1, Pt = _engine.Points(ctx, X0), _engine.Points(ctx, X1), _engine.Points(ctx, Xt)
    i0, w0 = _table(rng, 70, 4, 50)
    i1, w1 = _table(rng, 130, 9, 300)
    A0, A1 = mr.dense_of(i0, w0, 50), mr.dense_of(i1, w1, 300)
    T0, T1 = _engine.Mix(ctx, i0, w0, 50), _engine.Mix(ctx, i1, w1, 300)
    desc = _desc(lp, kernel, D, D)
    first = None
    for trip in range(2):
        M = _two_blocks(ctx, 70, 130)
        M.assemble_mixed(desc, P1, T1, P0, T0, 1, 0)
        G = M.todense("gram")[70:, :70]
        if first is None:
            first = G
            _hold("(a) 130 x 70, S0 = 9, S1 = 4", G, *mr.block(kernel, D, D, X1, X0, A1, A0), 9, 4)
    assert G.tobytes() == first.tobytes()        # no atomics: the same bits on every call
    # (c) rows mixed over 300 points against 50 plain points, and 130 plain rows against mixed columns
    M = _two_blocks(ctx, 50, 130)
    M.assemble_mixed(desc, P1, T1, P0, None, 1, 0)
    _hold("(c) mixed rows, plain columns", M.todense("gram")[50:, :50], *mr.block(kernel, D, D, X1, X0, A1, None), 9, 1)
    X2 = rng.uniform(-1, 1, (130, d))
    P2 = _engine.Points(ctx, X2)
    M = _two_blocks(ctx, 70, 130)
    M.assemble_mixed(desc, P2, None, P0, T0, 1, 0)
    _hold("(c) plain rows, mixed columns", M.todense("gram")[70:, :70], *mr.block(kernel, D, D, X2, X0, None, A0), 1, 4)
    # (e) the cross block
    ident = {(0, 0): 1.0}
    M = _two_blocks(ctx, 70, 130)
    rhs = _engine.Rhs(ctx, M, 33)
    rhs.cross_assemble_mixed(_desc(lp, kernel, D, ident), P1, T1, Pt, 1)
    _hold("(e) 130 x 33 cross block", rhs.to_host()[70:], *mr.block(kernel, D, ident, X1, Xt, A1, None), 9, 1)


@pytest.mark.parametrize("d,S", [(2, 32), (3, 32), (2, 19), (3, 11), (4, 9), (1, 17)])
def test_diagonal_block_at_the_cap_and_across_lds_chunks(lp, ctx, d, S):
    """(b) a 130-row diagonal block at S = 32, the cap: two full chunks of 16 slots at d = 2, four of 8 at d = 3; S = 19, 11, 9, 17: a
    ragged last chunk (3, 3, 1 and 1 slots).  Full rows, so that every slot of every chunk carries weight."""
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(1000 * d + S)
    kernel, D = _kernel(d), _lap(d)
    X = rng.uniform(-1, 1, (200, d))
    P = _engine.Points(ctx, X)
    idx, w = _table(rng, 130, S, 200, ragged=False)
    T = _engine.Mix(ctx, idx, w, 200)
    M = _two_blocks(ctx, 70, 130)
    M.assemble_mixed(_desc(lp, kernel, D, D), P, T, None, None, 1, 1)
    G = M.todense("gram")[70:, 70:]
    A = mr.dense_of(idx, w, 200)
    assert np.array_equal(G, G.T)
    _hold(f"(b) diagonal block, d = {d}, S = {S}", G, *mr.block(kernel, D, D, X, X, A, A), S, S)


def test_radial_and_wendland_descriptors_and_tiles_out_of_reach(lp, ctx, monkeypatch):
    """(d) An `LPGP_MATERN_RADIAL` descriptor (Laplacians on the isotropic Matern-5/2) and a Wendland descriptor with a support
    radius so small that whole 64 x 64 tiles are out of reach: rows 0 .. 63 draw their stencils from a cluster at the origin, the
    others from a cluster five units away, and the same for the columns.  The oracle has neither family, so the kernel values of the
    reference here are the device's own generic kernel on the points (`lpgp_kernel_matrix`, held to its references in
    tests/test_gpu_kernels.py and tests/test_gpu_wendland.py), mixed on the host.  The block is written over storage that holds
    another block's non-zero entries: the entries out of reach must be exactly 0.0 afterwards."""
    from linpde_gp_amd import _engine, _lib, config
    from linpde_gp_amd.linfuncops import diffops
    cf = lp.randprocs.covfuncs
    monkeypatch.setattr(config, "isotropic_matern_higher_order", True)          # Laplacians on the isotropic kernel: the radial family
    rng = np.random.default_rng(77)
    near, far = rng.uniform(0, 0.5, (100, 2)), 5.0 + rng.uniform(0, 0.5, (100, 2))
    X = np.concatenate([near, far])
    P = _engine.Points(ctx, X)

    def clustered(q, S):
        idx, w = _table(rng, q, S, 100)
        idx[64:] += 100                          # rows of the first tile over the near cluster, the others over the far one
        return idx, w
    i0, w0 = clustered(70, 4)
    i1, w1 = clustered(130, 9)
    T0, T1 = _engine.Mix(ctx, i0, w0, 200), _engine.Mix(ctx, i1, w1, 200)
    A0, A1 = mr.dense_of(i0, w0, 200), mr.dense_of(i1, w1, 200)
    kiso = cf.Matern((2,), nu=2.5, lengthscales=[0.7, 1.1])
    Lap = -1.0 * diffops.Laplacian((2,))
    kw = cf.WendlandCovarianceFunction((2,), 2, lengthscales=[0.9, 1.2])
    Dv = diffops.DirectionalDerivative([1.0, -0.5])
    filler = _desc(lp, _kernel(2), {(0, 0): 1.0}, {(0, 0): 1.0})
    P70, P130 = _engine.Points(ctx, rng.uniform(0, 1, (70, 2))), _engine.Points(ctx, rng.uniform(0, 1, (130, 2)))
    for name, kk in (("radial Matern-5/2, Laplacians", Lap(Lap(kiso, argnum=1), argnum=0)), ("Wendland d = 2, k = 2, directional derivatives", Dv(Dv(kw, argnum=1), argnum=0))):
        desc = kk.lower()
        assert any((_lib.MATERN_RADIAL if "radial" in name else _lib.WENDLAND_ISO) in g["family"] for g in desc), name
        K = _engine.kernel_matrix(ctx, desc, P, P)
        ref, env, absw = A1 @ K @ A0.T, np.abs(A1) @ np.abs(K) @ np.abs(A0).T, np.outer(np.abs(A1).sum(1), np.abs(A0).sum(1)) * np.abs(K).max()
        M = _two_blocks(ctx, 70, 130)
        M.assemble(filler, P130, P70, 1, 0)      # non-zero entries everywhere in the block's storage
        assert np.all(M.todense("gram")[70:, :70] > 0)
        M.assemble_mixed(desc, P, T1, P, T0, 1, 0)
        G = M.todense("gram")[70:, :70]
        _hold(f"(d) {name}", G, ref, env, absw, 9, 4)
        assert np.abs(G[:64, :64]).max() > 0 and np.abs(G[64:, 64:]).max() > 0
        if "Wendland" in name:
            assert np.all(K[:100, 100:] == 0.0)
            assert np.all(G[:64, 64:] == 0.0) and np.all(G[64:, :64] == 0.0)         # whole tiles out of reach: exact zeros, stored


# ---- posteriors through the public interface -----------------------------------------------------------------------------------
_cache = {}


def _problem(lp, name):
    if name not in _cache:
        if name.startswith("1d"):
            kernel, obs, Xt = mr.problem_1d("boundary first" if name == "1d boundary first" else "cells first")
            u, xt = mr.condition(lp, kernel, obs, scalar_input=True, sparse=name == "1d cells first"), Xt[:, 0]
        else:
            kernel, obs, Xt = mr.problem_2d()
            u, xt = mr.condition(lp, kernel, obs), Xt
        _cache[name] = (u, mr.Reference(kernel, obs), xt, Xt, obs)
    return _cache[name]


@pytest.mark.parametrize("name", ["1d boundary first", "1d cells first", "2d"])
def test_posterior_against_the_dense_reference(lp, ctx, name):
    u, R, xt, Xt, obs = _problem(lp, name)
    assert u._state.mat.block_sizes == [o.rows for o in obs] and (144 if name == "2d" else 140) in u._state.mat.block_sizes      # rows, not points
    assert [ob.rows for ob in u._blocks] == [o.rows for o in obs] and max(ob.points.n for ob in u._blocks) == (576 if name == "2d" else 420)
    mean, var = u.predict(xt)
    rm, rv = R.predict(Xt)
    ma, va = posterior_tolerances(rm, rv)
    em, ev = np.abs(mean - rm).max(), np.abs(var - rv).max()
    w = u.representer_weights
    ew, wa = np.abs(w - R.w).max(), POSTERIOR_RTOL * np.abs(R.w).max()
    print(f"{name}: n={R.r.size}  mean err {em:.3e} / {ma:.3e}   var err {ev:.3e} / {va:.3e}   weights err {ew:.3e} / {wa:.3e}")
    assert em <= ma and ev <= va and ew <= wa
    np.testing.assert_allclose(u.mean(xt), rm, rtol=0, atol=ma)
    np.testing.assert_allclose(u.std(xt) ** 2, rv, rtol=0, atol=va)
    cov = R.cov(Xt[:9])
    np.testing.assert_allclose(u.cov.matrix(xt[:9]), cov, rtol=0, atol=va)
    np.testing.assert_allclose(u.cov.linop(xt[:9]).todense(), cov, rtol=0, atol=va)


def test_downstream_of_the_factor(lp):
    """Evidence, leave-one-out and leave-block-out against the dense formulas on the reference G, with the tolerances
    tests/test_gpu_varcoef.py::test_downstream_of_the_factor holds the same factor to (POSTERIOR_RTOL relative to the quantity's
    largest entry, summed over the terms of a total)."""
    u, R, xt, _, obs = _problem(lp, "1d boundary first")
    n = R.r.size
    sign, logdet = np.linalg.slogdet(R.G)
    quad = float(R.r @ R.w)
    want = -0.5 * quad - 0.5 * logdet - 0.5 * n * np.log(2 * np.pi)
    lam = np.linalg.eigvalsh(R.G)
    slack = 2.0 * n * np.sqrt(3.0 * n + 1.0) * 2.0 ** -53 * lam[-1] * float(R.w @ R.w)        # tests/test_gpu_evidence.py: _quad_slack
    got = u.log_marginal_likelihood()
    print(f"lml {got:.15e} (ref {want:.15e}), slack {0.5 * slack + 0.5e-9 * abs(logdet):.3e}")
    assert sign == 1.0 and abs(got - want) <= 0.5 * slack + 0.5e-9 * abs(logdet)
    assert abs(u.gram.logabsdet() - logdet) <= 1e-9 * abs(logdet)
    Ginv = scipy.linalg.cho_solve((R.chol, True), np.eye(n))
    dd = np.diag(Ginv)
    loo = u.leave_one_out()
    loo_mean = R.r - R.w / dd                    # zero prior mean: y = r
    print(f"loo mean err {np.abs(loo.mean - loo_mean).max():.3e} / {POSTERIOR_RTOL * np.abs(loo_mean).max():.3e}")
    assert np.abs(loo.mean - loo_mean).max() <= POSTERIOR_RTOL * np.abs(loo_mean).max()
    offs = np.cumsum([0] + [o.rows for o in obs])
    logp = []
    for b in range(len(obs)):
        B = slice(offs[b], offs[b + 1])
        S = Ginv[B, B]
        wB = R.w[B]
        logp.append(-0.5 * wB @ np.linalg.solve(S, wB) + 0.5 * np.linalg.slogdet(S)[1] - 0.5 * (offs[b + 1] - offs[b]) * np.log(2 * np.pi))
    cv = u.cross_validate("blocks")
    print(f"cv total {cv.total:.12e} (ref {np.sum(logp):.12e})")
    assert [f.size for f in cv.folds] == [o.rows for o in obs]
    assert abs(cv.total - np.sum(logp)) <= POSTERIOR_RTOL * np.max(np.abs(logp)) * len(logp)
    assert u.sample(np.random.default_rng(0), xt, 3).shape == (3, 33)
    V = np.random.default_rng(1).standard_normal((n, 2))
    np.testing.assert_allclose(u.gram @ V, R.G @ V, rtol=0, atol=1e-11 * np.abs(R.G).max() * n)


def test_read_out_of_a_matrix_functional(lp):
    """`(A @ ev)(u)` for the posterior and the prior: `Normal(A m, A Sigma A^T)` from `u.mean` / `u.cov.matrix` on the points."""
    u, R, xt, Xt, _ = _problem(lp, "2d")
    rng = np.random.default_rng(5)
    A = np.where(rng.uniform(size=(7, 50)) < 0.2, rng.normal(size=(7, 50)), 0.0)
    ev = lp.linfunctls._EvaluationFunctional((2,), (), xt)
    for f in (u, u.prior):
        N = (A @ ev)(f)
        m = np.asarray(f.mean(xt), dtype=float)
        Sigma = f.cov.matrix(xt) if f is u else np.asarray(ev(f).cov)
        ma, va = posterior_tolerances(A @ m, A @ Sigma @ A.T)          # (the prior: A @ 0 must be exactly 0)
        assert np.asarray(N.mean).shape == (7,) and np.asarray(N.cov).shape == (7, 7)
        np.testing.assert_allclose(N.mean, A @ m, rtol=0, atol=ma)
        np.testing.assert_allclose(N.cov, A @ Sigma @ A.T, rtol=0, atol=va)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_python_refusals_that_need_a_context(lp, ctx, monkeypatch):
    from linpde_gp_amd import config
    u, _, xt, _, _ = _problem(lp, "1d boundary first")
    nblocks = u._state.mat.num_blocks
    x, A = mr.gauss_cells_1d(np.linspace(-0.5, 0.5, 6), 3)
    L = A @ lp.linfunctls._EvaluationFunctional((), (), x)
    with pytest.raises(NotImplementedError, match="A @ L"):
        u.log_marginal_likelihood_gradient()
    monkeypatch.setattr(config, "matrix_free_above", 100)
    with pytest.raises(NotImplementedError, match="matrix-free"):
        u.condition_on_observations(np.zeros(5), L=L)
    monkeypatch.setattr(config, "matrix_free_above", 0)
    monkeypatch.setattr(ctx, "distributed", True)              # what a context that joined a multi-GPU job says
    with pytest.raises(NotImplementedError, match="A @ L.*multi-GPU"):
        u.prior.condition_on_observations(np.zeros(5), L=L)
    with pytest.raises(NotImplementedError, match="A @ L.*multi-GPU"):
        u.condition_on_observations(np.zeros(5), L=L)
    monkeypatch.setattr(ctx, "distributed", False)
    assert u._state.mat.num_blocks == nblocks
    u2 = u.condition_on_observations(np.zeros(5), L=L, b=lp.randvars.Normal(np.zeros(5), np.full(5, 1e-2)))       # and the path itself still works
    assert np.all(np.isfinite(u2.mean(xt)))


def test_c_abi_refusals_leave_the_matrix_untouched(lp, ctx):
    import ctypes as C
    from linpde_gp_amd import _engine, _lib
    lib = _lib.lib
    rng = np.random.default_rng(6)
    X0, X1 = rng.uniform(-1, 1, (70, 2)), rng.uniform(-1, 1, (300, 2))
    P0, P1, P3 = _engine.Points(ctx, X0), _engine.Points(ctx, X1), _engine.Points(ctx, rng.uniform(-1, 1, (300, 3)))
    kd = _desc(lp, _kernel(2), {(0, 0): 1.0}, {(0, 0): 1.0})
    kd3 = _desc(lp, _kernel(3), {(0, 0, 0): 1.0}, {(0, 0, 0): 1.0})
    i1, w1 = _table(rng, 130, 9, 300)
    T1 = _engine.Mix(ctx, i1, w1, 300)
    T1short = _engine.Mix(ctx, i1[:100], w1[:100], 300)
    T1other = _engine.Mix(ctx, np.minimum(i1, 69), w1, 70)      # made for a set of 70 points
    M = _two_blocks(ctx, 70, 130)
    M.assemble(kd, P0, None, 0, 0); M.assemble_mixed(kd, P1, T1, P0, None, 1, 0); M.assemble_mixed(kd, P1, T1, None, None, 1, 1)
    M.add_diag(0, None, 1e-3); M.add_diag(1, None, 1e-3)
    before = M.todense("gram")
    # lpgp_mix_create
    h = C.c_void_p()
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    idx, w = np.ascontiguousarray(i1), np.ascontiguousarray(w1)
    wide_i, wide_w = np.zeros((4, 33), dtype=np.int32), np.ones((4, 33))
    over, neg = idx.copy(), idx.copy()
    over[7, 3], neg[7, 3] = 300, -1
    create = {
        "S = 0": lambda: lib.lpgp_mix_create(ctx._h, 130, 0, pi(idx), _lib.as_pd(w), 300, C.byref(h)),
        "S = 33": lambda: lib.lpgp_mix_create(ctx._h, 4, 33, pi(wide_i), _lib.as_pd(wide_w), 300, C.byref(h)),
        "an index at npts": lambda: lib.lpgp_mix_create(ctx._h, 130, 9, pi(over), _lib.as_pd(w), 300, C.byref(h)),
        "a negative index": lambda: lib.lpgp_mix_create(ctx._h, 130, 9, pi(neg), _lib.as_pd(w), 300, C.byref(h)),
        "null indices": lambda: lib.lpgp_mix_create(ctx._h, 130, 9, None, _lib.as_pd(w), 300, C.byref(h)),
        "null weights": lambda: lib.lpgp_mix_create(ctx._h, 130, 9, pi(idx), None, 300, C.byref(h)),
        "null result": lambda: lib.lpgp_mix_create(ctx._h, 130, 9, pi(idx), _lib.as_pd(w), 300, None),
    }
    for what, f in create.items():
        rc = f()
        msg = lib.lpgp_last_error().decode()
        assert rc != 0 and "lpgp_mix_create" in msg and not h.value, (what, rc, msg)
    # the assemblies
    ctx2 = _engine.Context(ctx.device)
    try:
        Tforeign = _engine.Mix(ctx2, i1, w1, 300)

        def gram(X0_=P1, M0=T1, X1_=P0, M1=None, bi=1, bj=0, kd_=kd):
            return lib.lpgp_gram_assemble_mixed(ctx._h, kd_, len(kd_), X0_._h, M0._h if M0 is not None else None, X1_._h if X1_ is not None else None,
                                                M1._h if M1 is not None else None, M._h, bi, bj)
        bad = {
            "q does not match the block": lambda: gram(M0=T1short),
            "a plain side of the wrong size": lambda: gram(M0=None),
            "a table made for another npts": lambda: gram(M0=T1other),
            "points of another dimension": lambda: gram(X0_=P3),
            "a descriptor of another dimension": lambda: gram(kd_=kd3),
            "a table of another context": lambda: gram(M0=Tforeign),
            "a column table on a diagonal block": lambda: gram(X1_=None, M1=T1, bj=1),
            "block above the diagonal": lambda: gram(bi=0, bj=1),
        }
        for what, f in bad.items():
            rc = f()
            msg = lib.lpgp_last_error().decode()
            assert rc != 0 and "lpgp_gram_assemble_mixed" in msg, (what, rc, msg)
            assert M.num_blocks == 2 and M.n == 200, what
        rhs = _engine.Rhs(ctx, M, 70)
        for what, T in (("q", T1short), ("npts", T1other), ("context", Tforeign)):
            assert lib.lpgp_cross_assemble_mixed(ctx._h, kd, len(kd), P1._h, T._h, P0._h, rhs._h, M._h, 1) != 0, what
            assert "lpgp_cross_assemble_mixed" in lib.lpgp_last_error().decode()
        assert lib.lpgp_cross_assemble_mixed(ctx._h, kd3, len(kd3), P1._h, T1._h, P0._h, rhs._h, M._h, 1) != 0
        del Tforeign
    finally:
        ctx2.close()
    assert np.array_equal(M.todense("gram"), before)            # nothing was written by any refused call
    # a factored block, and a strict-prefix view
    assert M.potrf() == 0
    factor = M.todense("factor")
    with pytest.raises(_lib.LpgpError, match="already factored"):
        M.assemble_mixed(kd, P1, T1, P0, None, 1, 0)
    M.add_block(130)
    M.assemble_mixed(kd, P1, T1, P0, None, 2, 0); M.assemble_mixed(kd, P1, T1, P1, T1, 2, 1); M.assemble_mixed(kd, P1, T1, None, None, 2, 2)
    M.add_diag(2, None, 1e-2)
    assert M.potrf() == 0
    M.set_view(2)
    with pytest.raises(_lib.LpgpError, match="strict prefix"):
        M.assemble_mixed(kd, P1, T1, P0, None, 1, 0)
    assert M.num_blocks == 2 and M.n == 200 and np.array_equal(M.todense("factor"), factor)
    M.set_view(-1)


def test_c_abi_refuses_a_context_inside_a_multi_gpu_job(lp, ctx):
    """A second context on the same device joins a job of one rank over the host-staged transport (`lpgp_dist_init_host`): from
    then on it is distributed, and the three entry points refuse it before they look at anything else."""
    import ctypes as C
    from linpde_gp_amd import _engine, _lib
    lib = _lib.lib
    ctx2 = _engine.Context(ctx.device)
    try:
        X = np.random.default_rng(8).uniform(-1, 1, (70, 2))
        kd = _desc(lp, _kernel(2), {(0, 0): 1.0}, {(0, 0): 1.0})
        P = _engine.Points(ctx2, X)
        T = _engine.Mix(ctx2, *_identity_table(70), 70)
        M = _engine.GramMatrix(ctx2)
        M.add_block(70)
        M.assemble(kd, P, None, 0, 0)
        before = M.todense("gram")
        rhs = _engine.Rhs(ctx2, M, 70)
        exchange = _lib.HOST_EXCHANGE_FN(lambda user, op, buf, nbytes, root: 0)
        _lib.check(lib.lpgp_dist_init_host(ctx2._h, 0, 1, exchange, None), "lpgp_dist_init_host")
        with pytest.raises(_lib.LpgpError, match="lpgp_gram_assemble_mixed: single GPU only"):
            M.assemble_mixed(kd, P, T, None, None, 0, 0)
        with pytest.raises(_lib.LpgpError, match="lpgp_cross_assemble_mixed: single GPU only"):
            rhs.cross_assemble_mixed(kd, P, T, P, 0)
        with pytest.raises(_lib.LpgpError, match="lpgp_mix_create: single GPU only"):
            _engine.Mix(ctx2, *_identity_table(70), 70)
        assert M.num_blocks == 1 and M.n == 70
        del rhs, M, P, T
    finally:
        ctx2.close()


def test_not_positive_definite_raises_and_the_earlier_posterior_is_intact(lp):
    u, _, xt, _, _ = _problem(lp, "1d cells first")
    u.representer_weights                                       # (both predictions below form the mean from the weights)
    u._pred_cache = None
    before = u.predict(xt)
    nblocks, n = u._state.mat.num_blocks, u._state.mat.n
    x, A = mr.gauss_cells_1d(np.linspace(-0.9, 0.9, 36), 3)
    A2 = np.repeat(A, 2, axis=0)                                # every row twice, no noise: singular
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        u.condition_on_observations(np.zeros(70), L=A2 @ lp.linfunctls._EvaluationFunctional((), (), x))
    assert u._state.mat.num_blocks == nblocks and u._state.mat.n == n
    u._pred_cache = None
    after = u.predict(xt)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
