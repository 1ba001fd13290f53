"""tests/_cv_reference.py (the long-double reference of test_gpu_cv.py) held to the DEFINITION of leave-fold-out prediction, and
the pure fold normalisation of `cross_validate`.  No GPU.

The reference evaluates the block formulas of GPML section 5.4.2 from a factor L: P = L^-T L^-1, S = P[B, B], mean_B = y_B -
S^-1 w_B, Sigma_B = S^-1, log p = -1/2 w_B^T S^-1 w_B + 1/2 log det S - b/2 log 2 pi.  The definition: delete the fold's rows and
columns from G, condition on the rest, predict the fold with its own noise.  Both in long double, on the oracle's dense Gram
matrix of a small two-block problem (40 values + 20 first derivatives under a Matern-5/2 prior, noise 1e-2).  So that the two
evaluate the SAME matrix to long-double accuracy the factor is NumPy's float64 Cholesky factor of the oracle's G and the
definition is applied to G' = L L^T formed in long double (G' = G up to a few float64 roundings per entry): the inversion of a
matrix of condition cond_2(G) by either route loses at most a small multiple of n eps cond_2(G) of the result, hence the bar
    max |a - b| <= 64 n eps_longdouble cond_2(G) max |b|     per quantity,
with cond_2(G) computed in the test and asserted <= 1e6 (the noise of 1e-2 is there for that).  Two identities besides: singleton
folds are the leave-one-out reference of _factor_reference.py, one fold of all rows is the evidence reference.

Before the GPU suite relies on it, the float64 yardstick of test_gpu_cv.py (the same formulas on LAPACK, `evaluate_float64`) is
held here to 1e-9 relative on that suite's problem and fold sets: otherwise its bar of 4 x the yardstick would show nothing."""
import numpy as np
import pytest

import _cv_reference as cv
import _factor_reference as fr
from oracle import gp as ogp

LD = fr.LD
EPS_LD = float(np.finfo(LD).eps)


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(60)
    X1, X2 = rng.uniform(-1, 1, (40, 1)), rng.uniform(-1, 1, (20, 1))
    Y1 = np.sin(3 * X1[:, 0]) + 0.1 * rng.standard_normal(40)
    Y2 = 3 * np.cos(3 * X2[:, 0]) + 0.1 * rng.standard_normal(20)
    blocks = [ogp.ObsBlock(X1, {(0,): 1.0}, Y1, None, 1e-2), ogp.ObsBlock(X2, {(1,): 1.0}, Y2, None, 1e-2)]
    G = ogp.gram(cv.Problem220.kernel, blocks)
    cond = float(np.linalg.cond(G))
    assert cond <= 1e6, cond
    L = np.linalg.cholesky(G)
    Gl = L.astype(LD) @ L.T.astype(LD)
    assert float(np.max(np.abs(Gl - G.astype(LD)))) <= 8 * 2.0 ** -53 * float(np.max(np.abs(G)))
    y = np.concatenate([Y1, Y2])
    r = y - 0.25                                   # (a constant prior mean of 0.25 on both blocks: r != y)
    return dict(G=Gl, L=L, r=r, y=y, n=60, tol=64 * 60 * EPS_LD * cond, cond=cond)


def close(a, b, tol, what):
    a, b = np.asarray(a).astype(LD), np.asarray(b).astype(LD)
    err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    print(f"{what}: {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def test_reference_against_the_definition(small):
    n = small["n"]
    perm = np.random.default_rng(7).permutation(n)
    cuts = np.cumsum([0, 1, 2, 5, 12, 30])         # 10 rows stay in no fold
    folds = [np.sort(perm[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert all(f.min() < 40 <= f.max() for f in folds[2:])
    got = cv.evaluate(small["L"], small["r"], small["y"], folds)
    print(f"cond_2(G) = {small['cond']:.3e}")
    rest = np.setdiff1d(np.arange(n), np.concatenate(folds))
    assert rest.size == 10 and np.all(np.isnan(got.mean[rest])) and np.all(np.isnan(got.var[rest]))
    logps = []
    for f, B in enumerate(folds):
        mean, Sigma, logp = cv.by_definition(small["G"], small["r"], small["y"], B)
        close(got.mean[B], mean, small["tol"], f"fold {f} ({B.size} rows) mean")
        close(got.var[B], np.diag(Sigma), small["tol"], f"fold {f} var")
        close(got.cov[f], Sigma, small["tol"], f"fold {f} cov")
        close([got.logp[f]], [logp], small["tol"], f"fold {f} log density")
        logps.append(logp)
    close([got.total], [sum(logps)], small["tol"], "total")


def test_singletons_are_leave_one_out(small):
    n = small["n"]
    got = cv.evaluate(small["L"], small["r"], small["y"], [np.array([i]) for i in range(n)])
    P, w = cv.inverse_and_weights(small["L"], small["r"])
    mean, var, logp = fr.loo(w, np.diag(P), small["y"])      # (long double in: astype keeps it)
    tol = 64 * EPS_LD                                         # the same P and w, scalar formulas: a few roundings
    close(got.mean, mean, tol * 4, "mean")
    close(got.var, var, tol, "var")
    close(got.logp, logp, tol * 4, "logp")
    close([got.total], [np.sum(logp)], tol * n, "total")
    assert all(c.shape == (1, 1) for c in got.cov)


def test_one_fold_of_all_rows_is_the_evidence(small):
    n = small["n"]
    got = cv.evaluate(small["L"], small["r"], small["y"], [np.arange(n)])
    z = fr.forward(small["L"], small["r"])
    logdet, _ = fr.logdet(np.diag(small["L"]))
    want = -LD(0.5) * (z @ z) - LD(0.5) * logdet - n * fr.HALF_LOG_2PI
    close([got.logp[0]], [want], small["tol"], "log marginal likelihood")
    assert got.total == got.logp[0]
    mean, Sigma, logp = cv.by_definition(small["G"], small["r"], small["y"], np.arange(n))
    close([logp], [want], small["tol"], "the definition with nothing left to condition on")
    close(got.cov[0], small["G"], small["tol"], "Sigma = G")
    # mean = y - r, where r has 17 digits and the reference's S^-1 w_B returns it through two inversions
    close(got.mean, small["y"] - small["r"], small["tol"], "mean = prior mean")


def test_the_float64_yardstick_of_the_gpu_suite_is_sharp():
    """test_gpu_cv.py allows the device 4 x the distance of the LAPACK evaluation from the long-double one, both from the
    device's factor; with NumPy's factor of the same Gram matrix standing in for the device's, that distance must be below 1e-9
    relative for every quantity on every fold set the suite uses -- and cond_2(G) <= 1e6."""
    p = cv.Problem220()
    G = p.gram()
    cond = float(np.linalg.cond(G))
    print(f"cond_2(G) = {cond:.3e}")
    assert G.shape == (220, 220) and cond <= 1e6
    L = np.linalg.cholesky(G)
    r = p.y.copy()
    a, b = p.boundary_folds()
    sets = {"mixed": p.mixed_folds(), "b128": a, "b129": b, "blocks": [np.arange(150), np.arange(150, 220)],
            "singletons": [np.array([i]) for i in range(220)], "all": [np.arange(220)]}
    assert [f.size for f in sets["mixed"]] == [1, 2, 16, 17, 127, 57] and np.array_equal(np.sort(np.concatenate(sets["mixed"])), np.arange(220))
    for name, folds in sets.items():
        ref, lap = cv.evaluate(L, r, p.y, folds), cv.evaluate_float64(L, r, p.y, folds)
        d = {"mean": cv.distance(lap.mean, ref.mean), "var": cv.distance(lap.var, ref.var), "logp": cv.distance(lap.logp, ref.logp),
             "total": cv.distance([lap.total], [ref.total]), "cov": max(cv.distance(x, y) for x, y in zip(lap.cov, ref.cov))}
        if name == "all":                         # zero prior mean: the exact mean is y - r = 0, no scale to be relative to
            assert float(np.max(np.abs(ref.mean))) < 1e-9 * float(np.max(np.abs(p.y)))
            del d["mean"]
        print(f"[{name}] float64 yardstick: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        assert max(d.values()) < 1e-9, (name, d)
        assert min(d.values()) > 0.0, "a yardstick of zero allows nothing"


# ---- the fold normalisation of cross_validate ----------------------------------------------------------------------------
def normalise(folds, sizes):
    from linpde_gp_amd.randprocs._gaussian_process import _normalise_folds
    return _normalise_folds(folds, sizes)


def test_normalise_folds_blocks_and_strides():
    fold_of, folds = normalise("blocks", [150, 70, 1])
    assert fold_of.dtype == np.int32 and fold_of.shape == (221,)
    assert np.array_equal(fold_of, np.repeat([0, 1, 2], [150, 70, 1]))
    assert [f.tolist() for f in folds] == [list(range(150)), list(range(150, 220)), [220]]
    fold_of, folds = normalise(8, [150, 70])
    assert np.array_equal(fold_of, np.arange(220) % 8) and len(folds) == 8
    assert all(np.array_equal(f, np.arange(k, 220, 8)) for k, f in enumerate(folds))
    fold_of, folds = normalise(np.int64(220), [150, 70])
    assert np.array_equal(fold_of, np.arange(220)) and len(folds) == 220
    assert len(normalise(2, [1, 1])[1]) == 2


def test_normalise_folds_explicit_lists():
    fold_of, folds = normalise([np.array([5, 3, 219]), [0], np.array([7], dtype=np.int32)], [150, 70])
    assert [f.tolist() for f in folds] == [[3, 5, 219], [0], [7]] and all(f.dtype == np.int64 for f in folds)
    want = np.full(220, -1)
    want[[3, 5, 219]], want[0], want[7] = 0, 1, 2
    assert np.array_equal(fold_of, want) and fold_of.dtype == np.int32
    fold_of, folds = normalise((range(0, 10), range(10, 20)), [20])
    assert np.array_equal(fold_of, np.repeat([0, 1], 10))


@pytest.mark.parametrize("folds,match", [
    ([[1, 2], [2, 3]], "overlaps"), ([[1, 1]], "twice"), ([[0], [220]], "outside"), ([[-1]], "outside"),
    ([[0], []], "empty"), ([], "no folds"), (1, "must lie in 2"), (221, "must lie in 2"), (0, "must lie in 2"), (-3, "must lie in 2"),
    ("edges", "blocks"), ([np.zeros((2, 2), dtype=int)], "1-D"), ([np.array([0.5, 1.0])], "integer"), (True, "sequence"), (2.5, "sequence"),
])
def test_normalise_folds_refusals(folds, match):
    with pytest.raises(ValueError, match=match):
        normalise(folds, [150, 70])


def test_fronts_without_a_factor_refuse():
    from linpde_gp_amd import _spawn
    from linpde_gp_amd.randprocs import _matrix_free
    with pytest.raises(NotImplementedError, match="`cross_validate` needs the dense factorisation"):
        _matrix_free.MatrixFreeConditionalGaussianProcess.cross_validate(None, "blocks")
    remote = [c for c in vars(_spawn).values() if isinstance(c, type) and "cross_validate" in vars(c)]
    assert len(remote) == 1
    with pytest.raises(NotImplementedError, match="`cross_validate` is not available through the `lp.spawn` multi-GPU front"):
        remote[0].cross_validate(None, 4)
