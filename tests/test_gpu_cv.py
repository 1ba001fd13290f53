"""Leave-fold-out cross-validation from the resident factor (csrc/evidence_cv.hip: `lpgp_mat_cv`) through `cross_validate()` and
the binding `GramMatrix.cv`, held to the DEVICE'S OWN factor: the reference (tests/_cv_reference.py, held to the definition in
test_cv_reference.py) evaluates the block formulas of GPML section 5.4.2 in long double from L as `todense("factor")` reads it
back, so the cond-bound error of the factorisation drops out (the method of test_gpu_evidence_backward.py).

One problem (`_cv_reference.Problem220`): prior Matern-5/2 in 1-D; 150 noisy values, then 70 noisy first derivatives at other
points, noise 1e-2; n = 220 in 256 + 128 = 384 padded rows, so the logical-to-padded map has a gap in the middle.

  1  mixed tile folds: a fixed permutation cut into folds of 1, 2, 16, 17, 127, 57 rows, each of more than one row across both blocks
  2  boundaries: a fold of exactly 128 rows (tile path); a fold of 129 rows (large path) beside one of 50; the other rows in no
     fold: NaN there, and nothing written outside the arrays handed over (128 + 129 rows do not fit into 220 disjointly: two calls)
  3  folds = "blocks": 150 rows on the large path, 70 on the tile path; an earlier posterior of the chain answers for its own block
  4  batching: "cv_fold_batch" = 3 on the 220 singletons (74 launches, the last of one fold): the bits of the default batch
  5  identities: singletons and `leave_one_out()`, one fold of all rows and `log_marginal_likelihood()`, each pair held to ONE reference
  6  determinism: two calls return the same bits; `predict` returns the same bits before and after (the resident weights stay)
  7  refusals: an unfactored matrix, a `ginv` of another layout, a `fold_of` entry out of range, an empty fold -- each an error, a
     correct call afterwards the bits of before; the byte counters show O(n) bytes without `return_cov`

  8  more folds than one trip takes: a second problem of 200 + 317 noisy values (517 rows in 256 + 384 padded) with 256, 257 and 517
     singleton folds, the other rows in no fold.  cv_total_kernel adds the log densities in fold order with one thread, 256 per trip
     of its loop (220 folds above: one trip), so `total` must be the left-to-right float64 sum of the device's own per-fold
     values bit for bit; 517 folds also cross the default "cv_fold_batch" = 512 without touching the option (two batches, the
     second of five folds), with the bits of batches of 3 and of 65535; per fold the reference and bar of 1 - 5; 517 singletons
     against `leave_one_out()` as in 5

Tolerance.  No a-priori bound for the tile Cholesky of S is derived here; the yardstick is measured: the same formulas in float64
on NumPy / SciPy (LAPACK) from the same device factor (`evaluate_float64`); its distance from the long-double reference, per
quantity (mean, var, log density per fold, total, covariances) and relative to the quantity's max-abs, is the yardstick, and the
device must stay within RATIO = 4 x that distance -- the margin tests/test_gpu_random.py grants against LAPACK, for two equally
valid float64 evaluations that sum in different orders.  The yardstick itself must be below 1e-9 relative (asserted; on the CPU
already in test_cv_reference.py), or the inputs would be too ill-conditioned to show anything.  One fold of all rows under a zero
prior mean has the exact mean 0: no scale to be relative to, so there the mean is held to 1e-9 max |y| instead.

Measured on the MI355X (every figure is printed by its test; MEASUREMENTS.md has the table), distance from the long-double
reference, device / LAPACK, worst quantity of each fold set:
  mixed 1.2e-14 / 1.3e-14 (var);  128 rows 2.2e-15 / 1.6e-15 (mean, 1.32 x);  129 + 50 rows 1.9e-15 / 1.5e-15 (mean, 1.24 x);
  "blocks" 2.1e-13 / 7.6e-14 (cov, 2.79 x; var 4.9e-14 / 1.8e-14 = 2.72 x, logp 1.46 x, total 1.19 x, mean 0.69 x);
  earlier posterior 1.4e-15 / 1.2e-15 (cov, 1.17 x);  singletons 1.9e-15 / 1.6e-15 (cov, 1.22 x), var at the yardstick itself;
  leave_one_out() at most 0.73 x;  all rows at most 0.96 x;  log_marginal_likelihood() 0.02 x.
  The tile path is within 1.32 x the yardstick everywhere, the large path within 2.79 x.

What the bar found while the code was written.  Every Cholesky factor of S here is computed with the Newton sign in the last
correction of a pivot's reciprocal square root (potrf_tile.h, `potrf_tile_body<true>`: the fold kernel, and potrf_tile_newton_kernel
for the large folds, with the resident panel chain kept off for that one factorisation).  With the sign the factorisation itself
carries (inv (1 - 1/2 inv^2 res) where the Newton step has +: the error the first step left is doubled, not removed, and scales the
whole column) the factor of S had a componentwise backward error of 11.7 u against LAPACK's 3.2 u, and the results read off S^-1
showed it: singleton variances 7.0 x the yardstick (82 u componentwise), the folds of the earlier posterior 4.6 x, the 150-row fold
of "blocks" (cond_2(S) = 5.4e3) 17 x in var and cov, 6.8 x in logp, 5.1 x in total."""
import ctypes as C
import functools
import operator

import numpy as np
import pytest

import _cv_reference as cv
from _backward import restored

pytestmark = pytest.mark.gpu

RATIO = 4.0
YARDSTICK_CAP = 1e-9


class Setup:
    def __init__(self):
        import linpde_gp_amd as lp
        from linpde_gp_amd import problems, randvars
        cf = lp.randprocs.covfuncs
        self.lp = lp
        self.p = p = cv.Problem220()
        prior = lp.GaussianProcess(lp.functions.Zero((1,)), cf.Matern((1,), nu=2.5, lengthscales=0.5))
        self.u1 = prior.condition_on_observations(p.Y[0], p.X[0], b=randvars.Normal(np.zeros(150), np.full(150, p.noise)))
        self.u2 = self.u1.condition_on_observations(p.Y[1], X=p.X[1], L=problems.operator_of(p.ops[1], 1), b=randvars.Normal(np.zeros(70), np.full(70, p.noise)))
        self.u2._check_current()
        self.mat = self.u2._state.mat
        self.ctx = self.mat.ctx
        assert self.mat.n == 220 and self.mat.padded_n == 384
        self.L = self.mat.todense("factor")
        self.r = self.u2._residual()
        assert np.array_equal(self.r, p.y)           # zero prior mean
        self._refs = {}

    def refs(self, name, folds, L=None, r=None, y=None):
        """(long-double reference, float64 LAPACK evaluation) of a fold set from the device's factor: computed once, never changed."""
        if name not in self._refs:
            L, r, y = (self.L, self.r, self.p.y) if L is None else (L, r, y)
            self._refs[name] = (cv.evaluate(L, r, y, folds), cv.evaluate_float64(L, r, y, folds))
        return self._refs[name]


@pytest.fixture(scope="module")
def s():
    setup = Setup()
    yield setup
    del setup.u2, setup.u1, setup.mat              # (the matrices go while the library is still loaded)


def hold(what, got, lap, ref, failures=None):
    """The device within RATIO x the yardstick.  `failures`: a list that takes the message instead of an assertion here, so that a
    test prints every figure before it fails."""
    dev, yard = cv.distance(got, ref), cv.distance(lap, ref)
    print(f"[{what}] device {dev:.3e}, LAPACK {yard:.3e}: ratio {dev / yard if yard else float('inf'):.2f}")
    assert 0.0 < yard < YARDSTICK_CAP, f"{what}: the float64 yardstick {yard:.3e} says nothing"
    if dev <= RATIO * yard:
        return
    msg = f"{what}: device {dev:.3e} = {dev / yard:.2f} x LAPACK's {yard:.3e} from the long-double reference"
    assert failures is not None, msg
    failures.append(msg)


def hold_all(name, got, lap, ref, folds, mean=True):
    """`got`: a FoldPredictions; every quantity against the yardstick, all figures printed first."""
    failures = []
    if mean:
        hold(f"{name} mean", got.mean, lap.mean, ref.mean, failures)
    hold(f"{name} var", got.var, lap.var, ref.var, failures)
    hold(f"{name} logp", got.log_predictive_density, lap.logp, ref.logp, failures)
    hold(f"{name} total", [got.total], [lap.total], [ref.total], failures)
    if got.cov is not None:
        assert len(got.cov) == len(folds) and all(c.shape == (f.size, f.size) for c, f in zip(got.cov, folds))
        dev = max(cv.distance(c, x) for c, x in zip(got.cov, ref.cov))
        yard = max(cv.distance(c, x) for c, x in zip(lap.cov, ref.cov))
        print(f"[{name} cov] device {dev:.3e}, LAPACK {yard:.3e}: ratio {dev / yard:.2f}")
        assert 0.0 < yard < YARDSTICK_CAP
        if dev > RATIO * yard:
            failures.append(f"{name} cov: device {dev:.3e} = {dev / yard:.2f} x LAPACK's {yard:.3e}")
        for c, f in zip(got.cov, folds):
            assert np.array_equal(c, c.T), "a covariance is not symmetric bit for bit"
            assert np.array_equal(np.diag(c), got.var[f]) or f.size > 128, "var is not the diagonal of the tile fold's covariance"
    assert not failures, "; ".join(failures)


def test_mixed_tile_folds(s):
    folds = s.p.mixed_folds()
    assert [f.size for f in folds] == [1, 2, 16, 17, 127, 57] and all(f.min() < 150 <= f.max() for f in folds[1:])
    got = s.u2.cross_validate(folds, return_cov=True)
    ref, lap = s.refs("mixed", folds)
    assert all(np.array_equal(a, b) for a, b in zip(got.folds, folds))
    assert got.mean.shape == got.var.shape == (220,) and got.log_predictive_density.shape == (6,)
    hold_all("mixed", got, lap, ref, folds)
    assert np.array_equal(got.std, np.sqrt(got.var))
    plain = s.u2.cross_validate(folds)
    assert plain.cov is None
    for a, b in ((plain.mean, got.mean), (plain.var, got.var), (plain.log_predictive_density, got.log_predictive_density), ([plain.total], [got.total])):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), "asking for the covariances changed the other results"


def raw_cv(s, fold_of, nfolds, want_cov, guard=8):
    """`lpgp_mat_cv` on arrays with `guard` sentinel doubles on either side; returns (mean, var, logp, cov) views, sentinels checked."""
    from linpde_gp_amd import _lib
    n, SENT = 220, -12345.678
    sizes = np.bincount(fold_of[fold_of >= 0], minlength=nfolds)
    lens = {"mean": n, "var": n, "logp": nfolds + 1, "cov": int(np.sum(sizes * sizes))}
    bufs = {k: np.full(v + 2 * guard, SENT) for k, v in lens.items()}
    view = {k: bufs[k][guard:guard + v] for k, v in lens.items()}
    ginv = s.mat.inverse()
    fo = np.ascontiguousarray(fold_of, dtype=np.int32)
    _lib.check(_lib.lib.lpgp_mat_cv(s.ctx._h, s.mat._h, ginv._h, _lib.as_pd(s.r), _lib.as_pd(s.p.y), fo.ctypes.data_as(C.POINTER(C.c_int32)), nfolds,
                                    _lib.as_pd(view["mean"]), _lib.as_pd(view["var"]), _lib.as_pd(view["logp"]),
                                    _lib.as_pd(view["cov"]) if want_cov else None), "lpgp_mat_cv")
    del ginv
    for k, b in bufs.items():
        assert np.all(b[:guard] == SENT) and np.all(b[guard + lens[k]:] == SENT), f"{k}: written outside the array"
    if not want_cov:
        assert np.all(bufs["cov"] == SENT)
    return view


def test_boundaries_128_and_129(s):
    a, b = s.p.boundary_folds()
    assert [f.size for f in a] == [128] and [f.size for f in b] == [129, 50]
    for name, folds in (("b128", a), ("b129", b)):
        got = s.u2.cross_validate(folds, return_cov=True)
        ref, lap = s.refs(name, folds)
        hold_all(name, got, lap, ref, folds)
        rest = np.setdiff1d(np.arange(220), np.concatenate(folds))
        assert rest.size == 220 - sum(f.size for f in folds) and np.all(np.isnan(got.mean[rest])) and np.all(np.isnan(got.var[rest]))
        assert np.all(np.isnan(got.std[rest]))
        fold_of = np.full(220, -1, dtype=np.int32)
        for f, idx in enumerate(folds):
            fold_of[idx] = f
        for want_cov in (True, False):
            raw = raw_cv(s, fold_of, len(folds), want_cov)
            assert raw["mean"].tobytes() == got.mean.tobytes() and raw["var"].tobytes() == got.var.tobytes()
            assert raw["logp"][:len(folds)].tobytes() == got.log_predictive_density.tobytes() and raw["logp"][len(folds)] == got.total
            if want_cov:
                assert raw["cov"].tobytes() == np.concatenate([c.reshape(-1) for c in got.cov]).tobytes()


def test_blocks(s):
    limit = s.ctx.get_option("chain_resident_max_rows")
    s.ctx.profile_enable(True)
    s.ctx.profile_reset()
    try:
        got = s.u2.cross_validate("blocks", return_cov=True)
        prof = s.ctx.profile_get()
    finally:
        s.ctx.profile_enable(False)
    # the large fold's 150 rows pad to two tiles, factored per tile (the Newton form has no resident chain); no option is touched for it
    assert prof["potrf_tile"]["launches"] == 2, prof["potrf_tile"]
    assert s.ctx.get_option("chain_resident_max_rows") == limit
    folds = [np.arange(150), np.arange(150, 220)]
    assert all(np.array_equal(a, b) for a, b in zip(got.folds, folds))
    ref, lap = s.refs("blocks", folds)
    hold_all("blocks", got, lap, ref, folds)


def test_the_earlier_posterior_answers_for_its_own_block(s):
    """The first posterior, asked after the second block was appended: its own 150 rows, strided into 5 tile folds."""
    got1 = s.u1.cross_validate(5, return_cov=True)
    assert s.mat.n == 150 and got1.mean.shape == (150,) and len(got1.folds) == 5
    L1 = s.mat.todense("factor")
    assert np.array_equal(L1, s.L[:150, :150])
    folds1 = [np.arange(k, 150, 5) for k in range(5)]
    ref1, lap1 = s.refs("earlier", folds1, L1, s.u1._residual(), s.p.Y[0])
    hold_all("earlier view", got1, lap1, ref1, folds1)
    s.u2._check_current()
    assert s.mat.n == 220


def test_batches_of_three_return_the_same_bits(s):
    folds = [np.array([i]) for i in range(220)]
    assert s.ctx.get_option("cv_fold_batch") == 512
    base = s.u2.cross_validate(folds, return_cov=True)
    with restored(s.ctx, ("cv_fold_batch",)) as apply:
        apply({"cv_fold_batch": 3})
        assert s.ctx.get_option("cv_fold_batch") == 3
        got = s.u2.cross_validate(folds, return_cov=True)
        for bad in (0, -1, 65536):
            with pytest.raises(Exception, match="cv_fold_batch must lie in 1 .. 65535"):
                s.ctx.set_option("cv_fold_batch", bad)
    assert s.ctx.get_option("cv_fold_batch") == 512
    for name in ("mean", "var", "log_predictive_density"):
        assert getattr(got, name).tobytes() == getattr(base, name).tobytes(), f"{name} depends on the batch size"
    assert got.total == base.total and np.array_equal(np.concatenate(got.cov), np.concatenate(base.cov))


def test_identities_loo_and_evidence(s):
    single = [np.array([i]) for i in range(220)]
    ref, lap = s.refs("singletons", single)
    got = s.u2.cross_validate(220, return_cov=True)          # k = n: row i is fold i
    assert all(np.array_equal(a, b) for a, b in zip(got.folds, single))
    hold_all("singletons", got, lap, ref, single)
    loo = s.u2.leave_one_out()
    hold("leave_one_out mean", loo.mean, lap.mean, ref.mean)
    hold("leave_one_out var", loo.var, lap.var, ref.var)
    hold("leave_one_out logp", loo.log_predictive_density, lap.logp, ref.logp)
    hold("leave_one_out total", [loo.total], [lap.total], [ref.total])
    everything = [np.arange(220)]
    ref, lap = s.refs("all", everything)
    got = s.u2.cross_validate(everything, return_cov=True)
    hold_all("all rows", got, lap, ref, everything, mean=False)
    assert float(np.max(np.abs(got.mean))) <= 1e-9 * float(np.max(np.abs(s.p.y)))      # the exact mean is y - r = 0
    assert got.total == got.log_predictive_density[0]
    hold("log_marginal_likelihood", [s.u2.log_marginal_likelihood()], [lap.total], [ref.total])


def test_bit_reproducible_and_the_resident_weights_stay(s):
    x = np.linspace(-1, 1, 37)[:, None]
    before = s.u2.predict(x)
    with pytest.raises(ValueError, match="overlaps"):         # (refused on the host, before anything is launched)
        s.u2.cross_validate(s.p.mixed_folds()[:5] + [np.arange(150, 220)])
    a = s.u2.cross_validate("blocks", return_cov=True)
    b = s.u2.cross_validate("blocks", return_cov=True)
    c, d = s.u2.cross_validate(s.p.mixed_folds(), return_cov=True), s.u2.cross_validate(s.p.mixed_folds(), return_cov=True)
    for p, q in ((a, b), (c, d)):
        for name in ("mean", "var", "log_predictive_density"):
            assert getattr(p, name).tobytes() == getattr(q, name).tobytes(), f"{name}: two calls differ"
        assert p.total == q.total and all(x_.tobytes() == y_.tobytes() for x_, y_ in zip(p.cov, q.cov))
    s.u2._pred_cache = None                                   # (a cached prediction would answer without the device)
    after = s.u2.predict(x)
    for p, q in zip(before, after):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes(), "predict changed: were the resident weights touched?"


def test_refusals_leave_everything_usable(s):
    from linpde_gp_amd import _engine
    from linpde_gp_amd._lib import LpgpError
    folds = s.p.mixed_folds()
    fold_of = np.full(220, -1, dtype=np.int32)
    for f, idx in enumerate(folds):
        fold_of[idx] = f
    ginv = s.mat.inverse()
    good = s.mat.cv(ginv, s.r, s.p.y, fold_of, 6)
    with pytest.raises(LpgpError, match="not .fully. factored"):
        ginv.cv(ginv, s.r, s.p.y, fold_of, 6)                 # the inverse is a plain matrix, not a factor
    other = _engine.GramMatrix(s.ctx, capacity_hint=256)
    other.add_block(220)
    with pytest.raises(LpgpError, match="another block layout"):
        s.mat.cv(other, s.r, s.p.y, fold_of, 6)
    del other
    bad = fold_of.copy()
    bad[17] = 6
    with pytest.raises(LpgpError, match=r"fold_of\[17\] = 6 is outside -1 .. 5"):
        s.mat.cv(ginv, s.r, s.p.y, bad, 6)
    bad[17] = -2
    with pytest.raises(LpgpError, match=r"fold_of\[17\] = -2"):
        s.mat.cv(ginv, s.r, s.p.y, bad, 6)
    with pytest.raises(LpgpError, match="fold 6 is empty"):
        s.mat.cv(ginv, s.r, s.p.y, fold_of, 7)
    with pytest.raises(LpgpError, match="0 folds"):
        s.mat.cv(ginv, s.r, s.p.y, fold_of, 0)
    again = s.mat.cv(ginv, s.r, s.p.y, fold_of, 6)
    del ginv
    for p, q in zip(good[:4], again[:4]):
        assert np.asarray(p).tobytes() == np.asarray(q).tobytes()
    assert good[4] is None and again[4] is None
    # what crosses the bus: O(n) bytes without the covariances -- at most 32 doubles per row -- and the covariances on top with them
    n = 220

    def moved(folds_, cov):
        h0, d0 = s.ctx.get_option("evidence_h2d_bytes"), s.ctx.get_option("evidence_d2h_bytes")
        s.u2.cross_validate(folds_, return_cov=cov)
        return s.ctx.get_option("evidence_h2d_bytes") - h0, s.ctx.get_option("evidence_d2h_bytes") - d0
    for name, folds_ in (("mixed", folds), ("blocks", "blocks"), ("singletons", 220)):
        up, down = moved(folds_, False)
        print(f"[bytes {name}] {up} up, {down} down without the covariances (n^2 doubles: {8 * n * n})")
        assert 0 < up <= 32 * 8 * n and 0 < down <= 32 * 8 * n
        up_c, down_c = moved(folds_, True)
        sizes = [f.size for f in folds] if name == "mixed" else ([150, 70] if name == "blocks" else [1] * n)
        assert down_c - down == 8 * sum(b * b for b in sizes) and up <= up_c <= up + 8 * (len(sizes) + 1)


# ---- 8: more than 256 folds, more than one default batch -------------------------------------------------------------------
class Setup517:
    """Prior Matern-5/2 (lengthscale 0.5) in 1-D, 200 then 317 noisy values at scattered points, noise 1e-2: 517 rows in 256 + 384
    padded rows.  The references of ALL 517 singleton folds are computed once; a singleton's result does not depend on which other
    rows are in folds, so the first nf of them are the reference of nf folds."""
    sizes = (200, 317)

    def __init__(self):
        import linpde_gp_amd as lp
        from linpde_gp_amd import randvars
        cf = lp.randprocs.covfuncs
        rng = np.random.default_rng(517)
        u = lp.GaussianProcess(lp.functions.Zero((1,)), cf.Matern((1,), nu=2.5, lengthscales=0.5))
        ys = []
        for nb in self.sizes:
            X = rng.uniform(-1.0, 1.0, (nb, 1))
            Y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(nb)
            u = u.condition_on_observations(Y, X, b=randvars.Normal(np.zeros(nb), np.full(nb, 1e-2)))
            ys.append(Y)
        self.u, self.y = u, np.concatenate(ys)
        u._check_current()
        self.mat = u._state.mat
        self.ctx = self.mat.ctx
        assert self.mat.n == 517 and self.mat.padded_n == 640
        L = self.mat.todense("factor")
        r = u._residual()
        assert np.array_equal(r, self.y)             # zero prior mean
        single = [np.array([i]) for i in range(517)]
        self.ref, self.lap = cv.evaluate(L, r, self.y, single), cv.evaluate_float64(L, r, self.y, single)

    def first(self, nf):
        """(reference, LAPACK evaluation) of the folds {0}, ..., {nf - 1}: NaN for the rows in no fold, the total in fold order."""
        out = []
        for res in (self.ref, self.lap):
            mean, var = res.mean.copy(), res.var.copy()
            mean[nf:], var[nf:] = np.nan, np.nan
            logp = res.logp[:nf]
            out.append(cv.CvResult(mean, var, logp, functools.reduce(operator.add, list(logp)), res.cov[:nf]))
        return out


@pytest.fixture(scope="module")
def s517():
    setup = Setup517()
    yield setup
    del setup.u, setup.mat


def same_bits(a, b, what):
    for name in ("mean", "var", "log_predictive_density"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), f"{name} {what}"
    assert a.total == b.total, f"total {what}"
    assert (a.cov is None) == (b.cov is None)
    if a.cov is not None:
        assert np.concatenate([c.reshape(-1) for c in a.cov]).tobytes() == np.concatenate([c.reshape(-1) for c in b.cov]).tobytes(), f"cov {what}"


@pytest.mark.parametrize("nf", [256, 257, 517])
def test_singleton_folds_beyond_one_trip_of_the_total(s517, nf):
    folds = [np.array([i]) for i in range(nf)]
    ref, lap = s517.first(nf)
    got = s517.u.cross_validate(folds, return_cov=True)
    assert got.log_predictive_density.shape == (nf,) and len(got.cov) == nf
    hold_all(f"{nf} singletons", got, lap, ref, folds)
    assert np.all(np.isnan(got.mean[nf:])) and np.all(np.isnan(got.var[nf:])) and np.all(np.isnan(got.std[nf:]))
    assert np.all(np.isfinite(got.mean[:nf])) and np.all(np.isfinite(got.var[:nf]))
    # the total: one thread, fold order -- the left-to-right float64 sum of the device's own values
    want = functools.reduce(operator.add, [float(v) for v in got.log_predictive_density])
    print(f"[{nf} singletons] total {got.total!r}, left-to-right sum of the device's logp {want!r}")
    assert got.total == want, f"total {got.total!r} is not the left-to-right sum {want!r} of the {nf} per-fold values"
    plain = s517.u.cross_validate(folds)
    assert plain.cov is None and plain.total == got.total and plain.log_predictive_density.tobytes() == got.log_predictive_density.tobytes()
    if nf == 517:
        # two batches at the default option (512 + 5 folds): the bits of batches of 3 and of one batch
        assert s517.ctx.get_option("cv_fold_batch") == 512
        with restored(s517.ctx, ("cv_fold_batch",)) as apply:
            for batch in (3, 65535):
                apply({"cv_fold_batch": batch})
                same_bits(s517.u.cross_validate(folds, return_cov=True), got, f"depends on the batch size ({batch} against 512)")
        assert s517.ctx.get_option("cv_fold_batch") == 512
        same_bits(s517.u.cross_validate(517, return_cov=True), got, "differs between k = n and the list of singletons")
        loo = s517.u.leave_one_out()
        hold("517 leave_one_out mean", loo.mean, lap.mean, ref.mean)
        hold("517 leave_one_out var", loo.var, lap.var, ref.var)
        hold("517 leave_one_out logp", loo.log_predictive_density, lap.logp, ref.logp)
        hold("517 leave_one_out total", [loo.total], [lap.total], [ref.total])
