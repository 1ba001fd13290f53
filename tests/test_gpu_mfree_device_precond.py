"""Matrix-free solves through the package with the preconditioner BUILT ON THE DEVICE (`config.matrix_free_device_preconditioner`:
`PivotedCholeskyPreconditioner._build_on_device` over `lpgp_pivchol_*`, `pcg_device` on `DevicePCG.from_resident`), held by the
bounds tests/test_gpu_mfree_solve.py takes from tests/_mfree_reference.py for the host-built one: converged, at most
`slack(it_ref)` iterations beyond the longdouble reference, true residual <= 2 rtol.  The kernels themselves are held step by step
in tests/test_gpu_pivchol.py; here: that the package reaches them, that the factor is never uploaded again, that the resident
iteration applies the same M^-1 bit for bit as one created from the downloaded factor, and the public read-out
`gram.pivoted_cholesky`."""
import numpy as np
import pytest

from oracle import covfuncs as ocf
from oracle import gp as ogp

import _mfree_reference as mr

pytestmark = pytest.mark.gpu

CONFIG_KEYS = ("matrix_free", "matrix_free_above", "matrix_free_preconditioner_rank", "matrix_free_rtol", "matrix_free_maxiter",
               "matrix_free_device_iteration", "matrix_free_rhs_chunk", "matrix_free_device_preconditioner")
GRID = [(k, n, z) for k in mr.KERNELS for z in mr.NOISES for n in mr.SIZES]
LAP = {(2, 0): -1.0, (0, 2): -1.0}


@pytest.fixture
def lp():
    import linpde_gp_amd
    saved = {k: getattr(linpde_gp_amd.config, k) for k in CONFIG_KEYS}
    linpde_gp_amd.config.matrix_free = True
    linpde_gp_amd.config.matrix_free_device_preconditioner = True
    yield linpde_gp_amd
    for k, v in saved.items():
        setattr(linpde_gp_amd.config, k, v)


def test_the_default_is_off():
    import linpde_gp_amd
    assert linpde_gp_amd.config.matrix_free_device_preconditioner is False


def _solve_and_check(lp, c, columns):
    lp.config.matrix_free_rtol = c.rtol
    u = mr.observe(lp, mr.prior(lp, c.kernel), c)
    X = u.gram.solve(np.array(c.B))
    info, pre = u.last_solve_info, u._precond
    it_ref, _ = mr.reference_iterations(c.kernel, c.n, c.noise, 200, columns)
    true = float(np.max(mr.true_residual(c.G, X, c.B)))
    print(f"{c} x {columns}: reference {it_ref}, device-built preconditioner (rank {pre.rank}) {info['iterations']} (slack {mr.slack(it_ref)}); "
          f"true residual / rtol {true / c.rtol:.3f}")
    assert pre._device is not None and pre._L is None          # built on the device, never downloaded by the solve
    assert pre.rank == len(set(pre.pivots.tolist())) <= min(200, c.n) and pre.delta > 0.0
    assert X.shape == c.B.shape
    assert info["device_resident"] is True and info["converged"]
    assert info["iterations"] <= it_ref + mr.slack(it_ref), (c, info["iterations"], it_ref)
    assert true <= 2.0 * c.rtol


@pytest.mark.parametrize("kernel,n,noise", GRID)
def test_solve_against_the_dense_reference(lp, kernel, n, noise):
    _solve_and_check(lp, mr.case(kernel, n, noise), mr.COLUMNS)


def test_solve_with_64_columns(lp):
    c = mr.case("matern52", 150, 1e-2, 64)
    assert c.B.shape == (150, 64)
    _solve_and_check(lp, c, 64)


def test_the_factor_is_never_uploaded_again(lp, monkeypatch):
    """The weights solve and a prediction in two variance chunks: three device solves, all on ONE resident factor; the uploading
    constructor of `DevicePCG` is not called once."""
    from conftest import POSTERIOR_RTOL
    from linpde_gp_amd import _engine
    real = _engine.DevicePCG
    uploads, residents = [], []

    class Spy(real):
        def __init__(self, *args, **kwargs):
            uploads.append(args)
            super().__init__(*args, **kwargs)

        @classmethod
        def from_resident(cls, pc, m, Sinv):
            residents.append((pc, m))
            return super().from_resident(pc, m, Sinv)

    monkeypatch.setattr(_engine, "DevicePCG", Spy)
    c = mr.case("matern52", 150, 1e-2)
    lp.config.matrix_free_rtol = c.rtol
    lp.config.matrix_free_rhs_chunk = 20
    u = mr.observe(lp, mr.prior(lp, c.kernel), c)
    w = u.representer_weights
    assert u.last_solve_info["device_resident"] is True
    Xt = np.random.default_rng(41).uniform(-1, 1, (37, 2))
    mean, var = u.predict(Xt)
    assert uploads == []
    assert [m for _, m in residents] == [1, 20, 17] and all(pc is u._precond._device for pc, _ in residents)
    assert float(np.max(mr.true_residual(c.G, w, c.B[:, 0]))) <= 2.0 * c.rtol
    post = ogp.condition(mr.KERNELS[c.kernel], [ogp.ObsBlock(c.X, ocf.identity(2), c.B[:, 0], 0.0, c.noise)])
    rm, rv = post.mean(Xt), post.var(Xt)
    em, ev = float(np.max(np.abs(mean - rm)) / np.max(np.abs(rm))), float(np.max(np.abs(var - rv)) / np.max(np.abs(rv)))
    print(f"predict with a device-built preconditioner: mean {em:.2e}, variance {ev:.2e} of the maximum (bar {POSTERIOR_RTOL:g})")
    assert em <= POSTERIOR_RTOL and ev <= POSTERIOR_RTOL


@pytest.mark.parametrize("n,rank", [(150, 17), (333, 200), (64, 200)])
def test_the_resident_iteration_applies_the_same_preconditioner_bit_for_bit(lp, n, rank):
    """`lpgp_pcg_create_pivchol` against `lpgp_pcg_create` fed the downloaded L: the same kernels on the same data, so Z = M^-1 R,
    P and the relative residuals of `lpgp_pcg_start` agree bit for bit."""
    from linpde_gp_amd import _engine
    from linpde_gp_amd.randprocs import _matrix_free as mfree
    c = mr.case("matern52", n, 1e-2)
    G = mr.observe(lp, mr.prior(lp, c.kernel), c)._G
    pre = mfree.PivotedCholeskyPreconditioner(G, rank)
    assert pre._device is not None and pre.rank == min(n, rank)
    Sinv = np.linalg.inv(pre._chol @ pre._chol.T)
    Sinv = 0.5 * (Sinv + Sinv.T)
    m = 3
    R = np.random.default_rng(43).standard_normal((n, m))
    bn = np.linalg.norm(R, axis=0)
    out = []
    for it in (_engine.DevicePCG.from_resident(pre._device, m, Sinv), _engine.DevicePCG(G.ctx, n, m, pre.L, Sinv, pre.delta)):
        Rd = _engine.DeviceVectors(G.ctx, n, m, R)
        Z, P = _engine.DeviceVectors(G.ctx, n, m), _engine.DeviceVectors(G.ctx, n, m)
        rel = it.start(Rd, Z, P, bn, 1e-10)
        out.append((Z.get(), P.get(), rel))
    assert np.any(out[0][0] != R / pre.delta)                   # (the low-rank part is applied)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_pivoted_cholesky_read_out(lp):
    """`u.gram.pivoted_cholesky(17)`: rank 17, distinct pivots, built on the device whatever the flag says -- and the pivots are those
    the host statement of the algorithm takes on the oracle's matrix."""
    lp.config.matrix_free_device_preconditioner = False
    c = mr.case("matern52", 150, 1e-2)
    u = mr.observe(lp, mr.prior(lp, c.kernel), c)
    f = u.gram.pivoted_cholesky(17)
    assert f._device is not None
    assert f.rank == 17 and f.L.shape == (17, 150) and f.L is f.L and f.delta > 0.0
    assert len(set(f.pivots.tolist())) == 17 and all(0 <= p < 150 for p in f.pivots)
    host, host_pivots = mr.build_preconditioner(c.G, 17)
    assert f.pivots.tolist() == host_pivots
    R = np.random.default_rng(47).standard_normal((150, 2))
    assert f.solve(R).shape == R.shape                           # (the host form works on the downloaded factor)
    assert u._precond is None                                    # a read-out: the posterior's own preconditioner is not touched
    full = u.gram.pivoted_cholesky()
    assert full.rank == 150 and sorted(full.pivots.tolist()) == list(range(150))
    with pytest.raises(ValueError):
        u.gram.pivoted_cholesky(-1)


def test_a_rank_beyond_the_device_cap_is_built_by_the_host_loop(lp, monkeypatch):
    """min(rank, n) above `LPGP_PIVCHOL_MAX_RANK` goes to the host loop, flag or not; the decision is held here with the Python-side
    constant lowered to 16 (the C refusal at 2 049 is in test_gpu_pivchol.py)."""
    from linpde_gp_amd import _lib
    assert _lib.PIVCHOL_MAX_RANK == 2048
    monkeypatch.setattr(_lib, "PIVCHOL_MAX_RANK", 16)
    c = mr.case("matern52", 64, 1e-2)
    u = mr.observe(lp, mr.prior(lp, c.kernel), c)
    at, above = u.gram.pivoted_cholesky(16), u.gram.pivoted_cholesky(17)
    assert at._device is not None and at.rank == 16
    assert above._device is None and above.rank == 17 and above.pivots[:16].tolist() == at.pivots.tolist()
    lp.config.matrix_free_rtol = c.rtol
    X = u.gram.solve(np.array(c.B))                              # rank setting 200 -> min(200, 64) = 64 > 16: host build, uploaded factor
    assert u._precond._device is None and u._precond.rank == 64 and u.last_solve_info["device_resident"] is True
    assert float(np.max(mr.true_residual(c.G, X, c.B))) <= 2.0 * c.rtol


def _blocks(lp, dense_noise):
    """The three-block operator of test_gpu_mfree_solve.py: (posterior, oracle G)."""
    from linpde_gp_amd.linfuncops import diffops
    rng = np.random.default_rng(23)
    n0, n1, n2 = 70, 130, 1
    X0, X1, X2 = rng.uniform(-1, 1, (n0, 2)), rng.uniform(-1, 1, (n1, 2)), np.array([[1.5, -1.5]])
    Y0, Y1, Y2 = rng.standard_normal(n0), rng.standard_normal(n1), rng.standard_normal(n2)
    nz0 = rng.uniform(1e-3, 1e-1, n0)
    if dense_noise:
        A = rng.standard_normal((n0, 3))
        nz0 = np.diag(nz0) + 1e-2 * (A @ A.T)
    u = mr.prior(lp, "matern52").condition_on_observations(Y0, X0, b=lp.randvars.Normal(np.zeros(n0), nz0))
    u = u.condition_on_observations(Y1, X1, L=-1.0 * diffops.Laplacian((2,)), b=lp.randvars.Normal(np.zeros(n1), 0.5))
    u = u.condition_on_observations(Y2, X2)
    blocks = [ogp.ObsBlock(X0, ocf.identity(2), Y0, 0.0, nz0), ogp.ObsBlock(X1, LAP, Y1, 0.0, 0.5), ogp.ObsBlock(X2, ocf.identity(2), Y2)]
    return u, ogp.gram(mr.KERNELS["matern52"], blocks)


def test_three_blocks_solve_with_a_device_built_preconditioner(lp):
    u, G = _blocks(lp, dense_noise=False)
    lp.config.matrix_free_rtol = rtol = mr.rtol_for(float(np.linalg.cond(G)))
    B = np.random.default_rng(29).standard_normal((G.shape[0], 3))
    X = u.gram.solve(B)
    info = u.last_solve_info
    true = float(np.max(mr.true_residual(G, X, B)))
    print(f"three blocks, device-built preconditioner (rank {u._precond.rank}): {info['iterations']} iterations, true residual / rtol {true / rtol:.3f}")
    assert u._precond._device is not None and 17 <= u._precond.rank <= 200
    assert info["device_resident"] is True and info["converged"] and true <= 2.0 * rtol


def test_a_dense_noise_block_builds_on_the_host_and_the_result_is_unchanged(lp):
    out = []
    for flag in (True, False):
        lp.config.matrix_free_device_preconditioner = flag
        u, G = _blocks(lp, dense_noise=True)
        lp.config.matrix_free_rtol = mr.rtol_for(float(np.linalg.cond(G)))
        B = np.random.default_rng(29).standard_normal((G.shape[0], 3))
        X = u.gram.solve(B)
        assert u._G.device_ok() is False and u._precond._device is None and "device_resident" not in u.last_solve_info
        out.append((X, u._precond.L, u._precond.delta, u.last_solve_info["iterations"]))
        f = u.gram.pivoted_cholesky(17)
        assert f._device is None and f.rank == 17
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2:] == out[1][2:]
