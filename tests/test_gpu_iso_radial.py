"""Second-order operators on isotropic Matern priors (the radial family, `LPGP_MATERN_RADIAL`) on the device: entry by entry against
the 50-digit goldens through every assembly path, the diagonal, posteriors, and a Poisson problem with a known solution.

Entry bound: |got - G| <= K eps E with E the golden's envelope and K = `_iso_radial_reference.K_DEVICE` = 4 x the worst
|err| / (eps E) of the NumPy fp64 helper against the same goldens (132.94, measured on the CPU: MEASUREMENTS.md).  The device
reaches 128.76 at worst on an MI355X (every path prints its figure)."""
import os

import numpy as np
import pytest

import _iso_radial_reference as ref
from conftest import posterior_tolerances

pytestmark = pytest.mark.gpu
EPS = 2.0**-53
OPS = ("lap_id", "id_lap", "lap_lap", "d01_lap", "mix_mix")


@pytest.fixture(scope="module")
def lp():
    import linpde_gp_amd
    return linpde_gp_amd


@pytest.fixture(scope="module")
def ctx(lp):
    from linpde_gp_amd import _engine
    return _engine.default_context()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "iso_radial.npz"))


@pytest.fixture()
def higher_order(lp):
    saved = lp.config.isotropic_matern_higher_order
    lp.config.isotropic_matern_higher_order = True
    yield
    lp.config.isotropic_matern_higher_order = saved


def operator_pairs(d, v):
    z = (0,) * d
    e = lambda i, k=1: tuple(k if j == i else 0 for j in range(d))  # noqa: E731
    ident = {z: 1.0}
    lap = {e(i, 2): 1.0 for i in range(d)}
    d01 = {tuple(1 if j < 2 else 0 for j in range(d)): 1.0}
    mix = {z: 2.0}
    for i in range(d):
        mix[e(i, 2)] = -0.5
        mix[e(i)] = float(v[i])
    return {"lap_id": (lap, ident), "id_lap": (ident, lap), "lap_lap": (lap, lap), "d01_lap": (d01, lap), "mix_mix": (mix, mix)}


def _check(what, got, G, E, full, full_ref, idx):
    """golden entries to K eps E, every entry of the block (the filler included) to 1e-12 max|block| against the helper"""
    sub = got[np.ix_(*idx)]
    err = np.abs(sub - G)
    ratio = float(np.max(err[E > 0] / (EPS * E[E > 0])))
    print(f"{what}: worst golden entry |err| / (eps E) = {ratio:.2f} (K = {ref.K_DEVICE:.2f}); filler "
          f"{np.abs(full - full_ref).max() / np.abs(full_ref).max():.2e} of max|block|")
    assert np.isfinite(full).all(), what
    assert (err <= ref.K_DEVICE * EPS * E).all(), (what, ratio)
    assert np.abs(full - full_ref).max() <= 1e-12 * np.abs(full_ref).max(), what


@pytest.mark.parametrize("d,p", [(d, p) for d in (2, 3) for p in (2, 3, 4)])
def test_blocks_against_the_goldens_through_every_assembly_path(lp, ctx, golden, higher_order, d, p):
    """The 24 x 24 golden points embedded in point sets of 70 and 130 (more than one 64-wide tile each way, ragged tails): rows of the
    130-set beyond the first tile, columns inside the first tile, so that both the rectangular block (130 x 70) and the lower
    triangle of the diagonal block (130 x 130) hold every golden pair."""
    from linpde_gp_amd import _engine
    cf = lp.randprocs.covfuncs
    tag = f"d{d}_nu{2 * p + 1}2"
    ls, X0g, X1g = golden[tag + "_lengthscales"], golden[tag + "_X0"], golden[tag + "_X1"]
    rng = np.random.default_rng(1000 * d + p)
    c_idx = np.sort(rng.choice(70, 24, replace=False))             # X1g inside the 70-set
    q_idx = np.sort(rng.choice(64, 24, replace=False))             # X1g inside the 130-set, first tile
    r_idx = np.sort(rng.choice(np.arange(64, 130), 24, replace=False))     # X0g inside the 130-set, later tiles
    A, B = rng.uniform(-1, 1, (70, d)), rng.uniform(-1, 1, (130, d))
    A[c_idx], B[q_idx], B[r_idx] = X1g, X1g, X0g
    PA, PB = _engine.Points(ctx, A), _engine.Points(ctx, B)
    k = cf.Matern((d,), nu=p + 0.5, lengthscales=ls)
    ops = operator_pairs(d, golden[tag + "_v"])
    descs = {name: cf.lower_groups(k._base_groups(), L0, L1) for name, (L0, L1) in ops.items()}
    tril = np.tril(np.ones((130, 130), dtype=bool))
    for name, (L0, L1) in ops.items():
        G, E = golden[f"{tag}_{name}"], golden[f"{tag}_{name}_E"]
        desc = descs[name]
        assert desc[0]["family"] == [4] * d
        ref_BA, ref_BB = ref.block(p, ls, L0, L1, B, A), ref.block(p, ls, L0, L1, B, B)
        # Gram assembly: rectangular block (1, 0) and the lower triangle of the diagonal block (1, 1)
        M = _engine.GramMatrix(ctx)
        M.add_block(70)
        M.add_block(130)
        M.assemble(desc, PA, None, 0, 0)
        M.assemble(desc, PB, PA, 1, 0)
        M.assemble(desc, PB, None, 1, 1)
        Gm = M.todense("gram")
        _check(f"{tag} {name} gram (1, 0)", Gm[70:, :70], G, E, Gm[70:, :70], ref_BA, (r_idx, c_idx))
        _check(f"{tag} {name} gram (1, 1) lower", Gm[70:, 70:], G, E, np.where(tril, Gm[70:, 70:], 0.0), np.where(tril, ref_BB, 0.0), (r_idx, q_idx))
        # cross assembly: rows of block 1 of K_Xx
        rhs = _engine.Rhs(ctx, M, 70)
        rhs.cross_assemble(desc, PB, PA, 1)
        Kx = rhs.to_host()[70:]
        _check(f"{tag} {name} cross", Kx, G, E, Kx, ref_BA, (r_idx, c_idx))
        # matrix-free product with the identity: every entry once, the other summands exact zeros
        Kmv = _engine.kernel_matvec(ctx, desc, PB, PA, np.eye(70))
        _check(f"{tag} {name} matvec", Kmv, G, E, Kmv, ref_BA, (r_idx, c_idx))
        del rhs, M
    # weighted assembly with two pairs; the weights are signed powers of two, so the products with them are exact and the golden
    # bound carries over with E = sum_p |w0 w1| E_p
    w0 = np.stack([2.0 ** rng.integers(-2, 3, 130) * rng.choice([-1.0, 1.0], 130), 2.0 ** rng.integers(-2, 3, 130) * rng.choice([-1.0, 1.0], 130)])
    w1 = np.stack([2.0 ** rng.integers(-2, 3, 70) * rng.choice([-1.0, 1.0], 70), 2.0 ** rng.integers(-2, 3, 70) * rng.choice([-1.0, 1.0], 70)])
    M = _engine.GramMatrix(ctx)
    M.add_block(70)
    M.add_block(130)
    M.assemble(descs["lap_lap"], PA, None, 0, 0)
    M.assemble_weighted([(descs["lap_lap"], 0, 0), (descs["mix_mix"], 1, 1)], w0, w1, PB, PA, 1, 0)
    Gw = M.todense("gram")[70:, :70]
    want = np.zeros((24, 24))
    env = np.zeros((24, 24))
    full_ref = np.zeros((130, 70))
    for q, name in enumerate(("lap_lap", "mix_mix")):
        W = np.outer(w0[q], w1[q])
        want += W[np.ix_(r_idx, c_idx)] * golden[f"{tag}_{name}"]
        env += np.abs(W[np.ix_(r_idx, c_idx)]) * golden[f"{tag}_{name}_E"]
        full_ref += W * ref.block(p, ls, *ops[name], B, A)
    _check(f"{tag} weighted, two pairs", Gw, want, env, Gw, full_ref, (r_idx, c_idx))


@pytest.mark.parametrize("d,p", [(2, 2), (3, 3), (4, 2)])
def test_diagonal_entries_equal_desc_diag(lp, ctx, higher_order, d, p):
    """Diagonal entries of a Gram block are what `lpgp_kernel_diag` (desc_diag) says, exactly, and finite; d = 4, nu = 5/2,
    (Lap, Lap) lowers and assembles: 40 x 40 against the helper."""
    from linpde_gp_amd import _engine
    cf = lp.randprocs.covfuncs
    ls = [0.9, 0.6, 1.3, 0.75][:d]
    lap = {tuple(2 if j == i else 0 for j in range(d)): 1.0 for i in range(d)}
    desc = cf.lower_groups(cf.Matern((d,), nu=p + 0.5, lengthscales=ls)._base_groups(), lap, lap)
    X = np.random.default_rng(40 + d).uniform(-1, 1, (40, d))
    P = _engine.Points(ctx, X)
    M = _engine.GramMatrix(ctx)
    M.add_block(40)
    M.assemble(desc, P, None, 0, 0)
    G = M.todense("gram")
    full = _engine.kernel_matrix(ctx, desc, P, P)
    diag = _engine.kernel_diag(ctx, desc)
    want = ref.block(p, ls, lap, lap, X, X)
    print(f"d={d} p={p}: diag {diag!r}; helper diag {want[0, 0]!r}; max err {np.abs(full - want).max() / np.abs(want).max():.2e} of max|block|")
    assert np.isfinite(diag) and np.isfinite(G).all()
    assert (np.diag(G) == diag).all() and (np.diag(full) == diag).all()
    assert abs(diag - want[0, 0]) <= 64 * EPS * abs(want[0, 0])      # (d^2 <= 16 positive summands, a few roundings each, in two orders)
    assert np.abs(full - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("lazy", [False, True], ids=["default", "lazy"])
def test_posterior_against_the_golden(lp, golden, higher_order, lazy):
    """64 collocation points under -Lap, then 32 boundary values with the 1e-8 nugget, 20 prediction points: the posterior solved
    in 50-digit mpmath (make_golden_iso_radial.py), under `posterior_tolerances`."""
    from linpde_gp_amd.linfuncops import diffops
    cf = lp.randprocs.covfuncs
    g = golden
    saved = lp.config.lazy_factorization
    lp.config.lazy_factorization = lazy
    try:
        prior = lp.GaussianProcess(lp.functions.Zero((2,)), float(g["post_scale"]) * cf.Matern((2,), nu=2.5, lengthscales=g["post_lengthscales"]))
        u = prior.condition_on_observations(g["post_Yc"], X=g["post_Xc"], L=-1.0 * diffops.Laplacian((2,)))
        u = u.condition_on_observations(g["post_Yb"], X=g["post_Xb"], b=lp.randvars.Normal(np.zeros(32), float(g["post_nugget"]) * np.eye(32)))
        mean, var = u.predict(g["post_Xt"])
    finally:
        lp.config.lazy_factorization = saved
    ma, va = posterior_tolerances(g["post_mean"], g["post_var"])
    em, ev = np.abs(mean - g["post_mean"]).max(), np.abs(var - g["post_var"]).max()
    print(f"lazy={lazy}: mean err {em:.3e} / {ma:.3e}   var err {ev:.3e} / {va:.3e}   cond {float(g['post_cond']):.2e}")
    assert em <= ma and ev <= va


def test_poisson_problem_with_known_solution(lp, higher_order):
    """-Lap u = 2 pi^2 sin(pi x) sin(pi y) on the unit square, u = 0 on the boundary: u = sin(pi x) sin(pi y).  600 scattered
    collocation points and 160 boundary points (more than four tiles), nu = 7/2: the truth lies inside the 2-sigma band;
    `sample`, `log_marginal_likelihood` and `leave_one_out` run on the same factor and are finite."""
    from linpde_gp_amd.linfuncops import diffops
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(7)
    Xc = rng.uniform(0.02, 0.98, (600, 2))
    t = (np.arange(40) + 0.5) / 40
    Xb = np.concatenate([np.column_stack([np.zeros(40), t]), np.column_stack([np.ones(40), t]), np.column_stack([t, np.zeros(40)]), np.column_stack([t, np.ones(40)])])
    f = 2 * np.pi**2 * np.sin(np.pi * Xc[:, 0]) * np.sin(np.pi * Xc[:, 1])
    prior = lp.GaussianProcess(lp.functions.Zero((2,)), cf.Matern((2,), nu=3.5, lengthscales=[0.35, 0.3]))
    u = prior.condition_on_observations(f, X=Xc, L=-1.0 * diffops.Laplacian((2,)))
    u = u.condition_on_observations(np.zeros(160), X=Xb, b=lp.randvars.Normal(np.zeros(160), 1e-8 * np.eye(160)))
    Xt = rng.uniform(0.05, 0.95, (50, 2))
    truth = np.sin(np.pi * Xt[:, 0]) * np.sin(np.pi * Xt[:, 1])
    mean, var = u.predict(Xt)
    std = np.sqrt(np.maximum(var, 0.0))
    print(f"Poisson: max |mean - truth| {np.abs(mean - truth).max():.3e}, max |mean - truth| / std {np.max(np.abs(mean - truth) / std):.3f}, std in [{std.min():.2e}, {std.max():.2e}]")
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert (np.abs(mean - truth) <= 2 * std).all()
    assert np.abs(mean - truth).max() < 1e-2
    draws = u.sample(np.random.default_rng(0), Xt[:10], size=3)
    assert draws.shape == (3, 10) and np.isfinite(draws).all()
    lml = u.log_marginal_likelihood()
    loo = u.leave_one_out()
    assert np.isfinite(lml) and np.isfinite(loo.mean).all() and np.isfinite(loo.var).all() and (loo.var > 0).all() and np.isfinite(loo.total)


def test_first_order_blocks_are_bit_identical_with_the_flag_on_and_off(lp, ctx):
    from linpde_gp_amd import _engine
    from linpde_gp_amd.linfuncops import diffops
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(3)
    P0, P1 = _engine.Points(ctx, rng.uniform(-1, 1, (70, 3))), _engine.Points(ctx, rng.uniform(-1, 1, (130, 3)))
    k = cf.Matern((3,), nu=2.5, lengthscales=[0.7, 1.1, 0.9])
    Dv, Dw = diffops.DirectionalDerivative([1.0, -0.5, 0.2]), diffops.DirectionalDerivative([0.3, 2.0, -1.0])
    out = {}
    saved = lp.config.isotropic_matern_higher_order
    for flag in (False, True):
        lp.config.isotropic_matern_higher_order = flag
        try:
            blocks = []
            for kk in (k, Dv(k, argnum=0), Dw(k, argnum=1), Dv(Dw(k, argnum=1), argnum=0)):
                desc = kk.lower()
                assert desc[0]["family"] == [3] * 3
                blocks.append(_engine.kernel_matrix(ctx, desc, P0, P1).tobytes())
                blocks.append(_engine.kernel_matvec(ctx, desc, P0, P1, np.eye(130)[:, :5]).tobytes())
            out[flag] = blocks
        finally:
            lp.config.isotropic_matern_higher_order = saved
    assert out[False] == out[True]
