"""csrc/evidence.hip and the forward half of the single-vector solve that only it uses (trsv.hip solve_vec_fwd_resident, potrf.hip
solve_vec_fwd), held to the DEVICE'S OWN factor: every reference is computed in long double (tests/_factor_reference.py, itself
checked against 50-digit mpmath in test_factor_reference.py) from L as `todense("factor")` and `factor_diag()` read it back, so
the cond-bound error of the factorisation drops out and a measure sees these kernels alone (the method of
test_gpu_predict_backward.py for V = L^-1 K).  test_gpu_evidence.py keeps the end-to-end comparison with the oracle's Gram matrix.

  a  z = L^-1 r (the hook lpgp_test_solve_vec_fwd: the staging and the dispatch of lpgp_mat_evidence): componentwise backward
     error max_i |r - L z|_i / (|L||z| + |r|)_i <= RATIO_Z[form] x scipy.linalg.solve_triangular's on the same L and r; padding
     entries exactly 0.0; two runs of one mode give the same bytes.
  b  r^T G^-1 r = `evidence(r)[0]` against the long-double sum of squares of the SAME z (the kernels are deterministic), at the
     a-priori bound of evidence_partial_kernel + evidence_final_kernel.  For pn <= 65 536 = 256 workgroups x 256 threads a thread
     holds at most one row, and a path from a term to the result has 17 roundings: 1 fma (z^2 + 0), 6 shuffle adds, 2 adds over
     the four waves in stage 1; the partial read as it is, 6 shuffle adds, 2 adds over the waves in stage 2.  All terms are
     non-negative, so |q - sum z^2| <= ((1 + u)^17 - 1) q < SUM_ULPS u q with SUM_ULPS = 20.
  c  log det = `evidence(r)[1]` against 2 sum log L_ii in long double from factor_diag(), ABSOLUTE against u 2 sum |log L_ii|
     (noise "s" makes the logs change sign: |log det| is as small as 0.28 of that sum).  The same 17 roundings (the per-thread
     add is 0 + log: exact; the final doubling is exact) plus the device log's own error: LOG_ULPS, set from the measurement.
  d  diag(G^-1) = `inverse_diag()`: maximum componentwise relative error against d = colsum(W * W), W = L^-1 in long double,
     <= RATIO_D x the same measure of LAPACK (solve_triangular(L, I), column sums of squares in double) on the same L; panels
     of 128, 256 and 4096 columns (panel boundaries on and off block boundaries, padding rows inside panels, every panel after
     the first solved against a trailing sub-factor).  On noise "s" d must span at least eight decades: the normwise bar of
     test_gpu_evidence.py sees only the top of that range.
  e  the LOO epilogue, entry-tight, on the device's own w = `solve_weights(r)` and d = `inverse_diag()`:
       var   == 1 / d bit for bit (fp64 division is correctly rounded; the build has no fast-math);
       mean  = fl(y - fl(w fl(1 / d))): three roundings, |mean - (y - w / d)| <= u (2 |w / d| + |y - w / d|) to first order;
       logp  = fl(fl(1/2 fl(log d) - 1/2 w step) - c), step = fl(w fl(1 / d)), c = fl(1/2 log 2 pi):
               |logp - exact| <= u ((LOG_ULPS + 2) |1/2 log d| + 5 (1/2 w^2 / d) + 2 c)   (the log's share as in c; the product
               carries the two roundings of step and its own; two subtractions, each bounded by the sum of the moduli of its
               terms; the constant's rounding; a contraction into an fma only removes roundings);
       total against the long-double sum of the device's logp over the LOGICAL rows: 17 roundings as in b, <= SUM_ULPS u sum |logp|.
  f  the LOO variance and std through the public `leave_one_out()` on noise "s", componentwise against 1 / d and sqrt(1 / d) from
     the device's L, at the bar of d (LAPACK's d through the same two formulas).

  g  the second regime of the reductions of b, c and e: beyond 65 536 padded rows (the README's c4) a thread of evidence_partial_kernel
     and loo_epilogue_kernel takes several rows, i = b 256 + t, + 256 nwg, ...  The hooks lpgp_test_evidence and lpgp_test_loo cap the
     workgroups at 1 and 2, so that at 768 padded rows ("n700", "chain") a thread holds k = ceil(pn / (256 nwg)) = 3 and 2 rows.  The
     references are those of b, c and e; the bounds follow the depth (tests/_factor_reference.py, held on the CPU in
     test_factor_reference.py; at k = 1 they are the constants above):
       b, e-total: a thread adds its k terms by k fmas (adds), one rounding each, the first onto 0.0; the two stages as in b: 16 + k
               roundings on a path, |q - sum z^2| <= ((1 + u)^(16 + k) - 1) q < sum_ulps(k) u q, sum_ulps(k) = 19 + k (20 at k = 1);
       c:      the thread's first add 0 + log is exact, each of its k - 1 further adds rounds once, by at most u x the moduli it has
               added: log_ulps(k) = LOG_ULPS + (k - 1) in u 2 sum |log L_ii|;
       e, per row: mean, var and logp do not depend on the grid: the bits of the uncapped call.
     Exact case: the identity factor in the layout of the chain, r integers of [-8, 8]: z = r, every z^2 and every partial sum an
     integer, log 1 = 0: `evidence` returns (sum r^2, 0.0) exactly for 1, 2 and all workgroups.
     The status EV_NAN_PADDING ("a padding row of the factor is not a row of the identity"): the diagonal entry of one padding row
     set to 2.0 through lpgp_test_mat_raw makes `evidence` raise; with one workgroup and a padding row beyond row 255 the count is
     carried over the trips of the thread's loop; with the entry restored the call returns the bits of before.  A checked error
     return: nothing faults.

Matrices (tests/_backward.py Appender): Matern-5/2, lengthscale 0.3, scattered points of [0, 1]^2, noise "m" (1: the easy
control), "b" (1e-8: condition ~1e10) and "s" (rows over twelve decades); for z also "h", noise "b" on the points of [0, 0.5]^2
(the worst diagonal tile of L has cond >= 1e4 at 700 rows: a tile solve without its refinement step shows).  The right-hand
side r is a smooth function of the points, as the residual of a conditioning is.  Layouts: one block of 100, 128, 300, 700 rows; the
chain 150 + 70 + 1 + 200 (6 tile rows, tails of 106, 58, 127, 56 padded rows); the earlier view, the first two blocks of that
chain asked after all four were appended and factored; for z alone also 1600 and 4700 rows (13 and 37 tile rows).

Measured on the MI355X (every figure is printed by its test; MEASUREMENTS.md has the table):
  RATIO_Z   largest device / LAPACK ratio: resident 1.51 (m, 128 rows), per tile row 2.70 (m, 100 rows: 3.4 u against 1.3 u; the
            per-tile form chains 32 products per thread, the resident one 16); from 1600 rows on both are below 0.8
  RATIO_D   largest device / LAPACK ratio 1.20 (b, 128 rows; the same for every panel width); public var 1.08, std 1.00
  LOG_ULPS  largest |log det - ref| / (u 2 sum |log L_ii|) 1.85 (b, 300 rows); the log's share that logp needs: 0.12
  b: at most 0.16 of the bound; e: mean 0.99 (a correctly rounded result may sit at the bound), logp 0.55, total 0.07 of their bounds.
Defect runs (recorded, not tests; one scratch build each, in-bounds):
  no refinement step in the resident solve (LPGP_TRSV_FLAGS=1, fresh process): 14 of the 26 resident cases of a fail, ratios
    3.0 - 32.9 (b, 100 rows) where the unchanged kernel has 0.45 - 1.51; the dense points "h" 6.5 and 4.9 against 0.75 and 0.48.
    Noise "b" on [0, 1]^2 alone is too easy from 700 rows on (worst tile cond 2.3e3: 2.4 x LAPACK's at 700 rows, 1.9 at 4700, where
    LAPACK's own error has grown to 12 u) -- hence "h", the points of test_gpu_predict_backward.py (cond 1.8e4 at 700 rows);
  col_sumsq_lower_kernel starts two rows late: all 54 cases of d fail, and f and e with them (the last column sums nothing: d = 0);
  col_sumsq_lower_kernel makes one pass (`for` -> `if`): the 18 cases of d and 3 of f with more than 512 padded rows fail
    (relative error 3e-2 and more); e passes, as it must: lpgp_mat_loo and lpgp_mat_inverse_diag run the same launches;
  loo_epilogue_kernel ignores lrow in the sum: 90 of the 108 cases of e fail on `total` (1e11 - 1e14 x the bound); the 18 that
    pass are the 128-row layout, which has no padding row."""
import numpy as np
import pytest
import scipy.linalg

import _factor_reference as fr
from _backward import Appender, gram_points, restored

pytestmark = pytest.mark.gpu

U = fr.U
LD = fr.LD
RATIO_Z = {1: 3.0, 0: 5.0}     # a: backward error of z <= RATIO_Z[trsv_resident] x solve_triangular's  (<= twice the largest measured)
RATIO_D = 2.4          # d, f: relative error of diag(G^-1) <= RATIO_D x LAPACK's           (<= twice the largest measured ratio)
SUM_ULPS = 20.0        # b, c, e: 17 roundings on a path of the two-stage reductions
LOG_ULPS = 7.0         # c, e: reduction + device log, in u 2 sum |log L_ii| (<= 4 x the largest measured, never above 32)
HALF_LOG_2PI = 0.91893853320467274178

CHAIN = [150, 70, 1, 200]
SMALL = {"n100": ([100], None), "n128": ([128], None), "n300": ([300], None), "n700": ([700], None), "chain": (CHAIN, None),
         "view": (CHAIN, 2)}
LARGE = {"n1600": ([1600], None), "n4700": ([4700], None)}
KINDS = ["m", "b", "s"]
PANELS = [128, 256, 4096]


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    yield _engine.default_context()
    _cases.clear()                  # (the matrices go while the library is still loaded)


@pytest.fixture
def opts(ctx):
    with restored(ctx, ("trsv_resident", "inverse_diag_panel")) as apply:
        yield apply


def padded(nb):
    return -(-nb // 128) * 128


class Case:
    """Blocks appended and factored one by one as a conditioning does, then (view) the leading `view` blocks asked; the factor
    of what is in view read back.  The long-double references are computed once, on first use, and never changed."""

    def __init__(self, ctx, kind, blocks, view):
        self.kind = kind
        X, noise = gram_points("b" if kind == "h" else kind, sum(blocks))
        self.ap = Appender(ctx, 0.5 * X if kind == "h" else X, noise)
        for nb in blocks:
            self.ap.add(nb)
            assert self.ap.mat.potrf() == 0
        self.mat = self.ap.mat
        if view is not None:
            self.mat.set_view(view)
            blocks = blocks[:view]
        self.blocks, self.n = list(blocks), sum(blocks)
        assert self.mat.n == self.n and self.mat.padded_n == sum(padded(nb) for nb in blocks)
        self.rows = np.concatenate([poff + np.arange(nb) for nb, poff in zip(blocks, np.cumsum([0] + [padded(nb) for nb in blocks]))])
        self.L = self.mat.todense("factor")
        self.diag = self.mat.factor_diag()
        assert np.array_equal(self.diag, np.diag(self.L))
        # the residual of a smooth function, as a conditioning has it: z = L^-1 r then cancels inside every tile solve, which
        # is where a lost refinement step shows (with a standard normal r, noise "b" stays within 1.4 x LAPACK's from 700 rows on)
        Xv = X[:self.n]
        self.r = np.sin(3.0 * Xv[:, 0]) * np.cos(2.0 * Xv[:, 1]) + 0.5
        self.y = np.random.default_rng(self.n + 1).standard_normal(self.n)
        self._ref, self.logdet = {}, {}

    def once(self, key, make):
        if key not in self._ref:
            self._ref[key] = make()
        return self._ref[key]

    @property
    def z_lapack_error(self):
        return self.once("z", lambda: fr.backward_error(self.L, scipy.linalg.solve_triangular(self.L, self.r, lower=True), self.r))

    @property
    def d_ref(self):
        return self.once("d", lambda: fr.inverse_diag(fr.inverse(self.L)))

    @property
    def d_lapack(self):
        def make():
            W = scipy.linalg.solve_triangular(self.L, np.eye(self.n), lower=True)
            return np.sum(W * W, axis=0)
        return self.once("dl", make)


_cases = {}


def case(ctx, kind, layout):
    """The small cases are kept for the whole module; of the large ones (z alone) only the last."""
    key = (kind, layout)
    if key not in _cases:
        for k in [k for k in _cases if k[1] in LARGE]:
            del _cases[k]
        _cases[key] = Case(ctx, kind, *(SMALL.get(layout) or LARGE[layout]))
    return _cases[key]


def worst(values):
    i = int(np.argmax(values))
    return float(values[i]), i


# ---- a: the forward half -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [1, 0], ids=["resident", "per_tile"])
@pytest.mark.parametrize("kind,layout", [(k, la) for k in KINDS for la in list(SMALL) + list(LARGE)] + [("h", "n700"), ("h", "n1600")])
def test_forward_solve_backward_error(ctx, opts, kind, layout, resident):
    import _hooks
    c = case(ctx, kind, layout)
    opts({"trsv_resident": resident})
    zp = _hooks.solve_vec_fwd(ctx, c.mat, c.r)
    assert zp.shape == (c.mat.padded_n,) and np.all(np.isfinite(zp))
    pad = np.ones(zp.size, dtype=bool)
    pad[c.rows] = False
    assert np.all(zp[pad] == 0.0), "a padding entry of z is not exactly 0.0"
    again = _hooks.solve_vec_fwd(ctx, c.mat, c.r)
    assert zp.tobytes() == again.tobytes(), "two runs of one mode differ: no atomics in these solves, a difference is a race"
    be, be_ref = fr.backward_error(c.L, zp[c.rows], c.r), c.z_lapack_error
    print(f"\n[z {kind} {layout} resident={resident}] backward error {be / U:.2f} u (solve_triangular {be_ref / U:.2f} u): ratio {be / be_ref:.3f}")
    assert be <= RATIO_Z[resident] * be_ref, f"backward error of z {be / U:.2f} u = {be / be_ref:.2f} x solve_triangular's {be_ref / U:.2f} u"


def test_the_dense_points_make_the_diagonal_tiles_ill_conditioned(ctx):
    """Without cond(L_jj) >= 1e4 a tile solve that lost its refinement step passes the bar of z from 700 rows on (noise "b" on
    [0, 1]^2: 2.3e3 at 700 rows)."""
    c = case(ctx, "h", "n700")
    conds = [np.linalg.cond(c.L[i:i + 128, i:i + 128]) for i in range(0, c.n, 128)]
    print(f"\nworst diagonal tile of L (h, 700 rows): cond {max(conds):.2e}")
    assert max(conds) >= 1e4


# ---- b, c: the two terms of the evidence -----------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [1, 0], ids=["resident", "per_tile"])
@pytest.mark.parametrize("layout", list(SMALL))
@pytest.mark.parametrize("kind", KINDS)
def test_evidence_terms(ctx, opts, kind, layout, resident):
    import _hooks
    c = case(ctx, kind, layout)
    assert c.mat.padded_n <= 65536                     # (a thread of the reductions holds at most one row: the count of 17)
    opts({"trsv_resident": resident})
    zp = _hooks.solve_vec_fwd(ctx, c.mat, c.r)
    q, logdet = c.mat.evidence(c.r)
    q_ref = np.sum(zp.astype(LD) ** 2)
    eq = float(abs(LD(q) - q_ref) / (SUM_ULPS * U * q_ref))
    ld_ref, scale = fr.logdet(c.diag)
    el = float(abs(LD(logdet) - ld_ref) / (U * scale))
    print(f"\n[evidence {kind} {layout} resident={resident}] q {q:.17e}: {eq:.3f} of the bound; log det {logdet:.17e} "
          f"({float(ld_ref / scale):+.2f} of 2 sum |log|): {el:.3f} u 2 sum |log L_ii|")
    assert eq <= 1.0, f"r^T G^-1 r is {eq:.2f} x the bound of its reduction from the sum of squares of z"
    assert el <= LOG_ULPS, f"log det is {el:.2f} u 2 sum |log L_ii| from 2 sum log L_ii"
    c.logdet[resident] = logdet
    assert len(set(c.logdet.values())) == 1, "log det depends on the form of the solve"


# ---- d: the inverse diagonal ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel", PANELS, ids=[f"panel{p}" for p in PANELS])
@pytest.mark.parametrize("layout", list(SMALL))
@pytest.mark.parametrize("kind", KINDS)
def test_inverse_diag_componentwise(ctx, opts, kind, layout, panel):
    c = case(ctx, kind, layout)
    opts({"inverse_diag_panel": panel})
    d = c.mat.inverse_diag()
    assert d.shape == (c.n,) and np.all(np.isfinite(d)) and np.all(d > 0)
    ref = c.d_ref
    rel = np.abs(d.astype(LD) - ref) / ref
    e, i = worst(rel)
    e_ref = fr.relative_error(c.d_lapack, ref)
    span = float(np.log10(float(ref.max() / ref.min())))
    print(f"\n[d {kind} {layout} panel={panel}] relative error {e / U:.1f} u at row {i} (d = {float(ref[i]):.2e}; LAPACK {e_ref / U:.1f} u): "
          f"ratio {e / e_ref:.3f}; d over {span:.1f} decades")
    assert e <= RATIO_D * e_ref, f"diag(G^-1) row {i}: {e / U:.1f} u = {e / e_ref:.2f} x LAPACK's {e_ref / U:.1f} u"
    if kind == "s":
        assert span >= 8.0, "noise s no longer spreads diag(G^-1) over eight decades"


# ---- e: the leave-one-out epilogue ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [1, 0], ids=["resident", "per_tile"])
@pytest.mark.parametrize("panel", PANELS, ids=[f"panel{p}" for p in PANELS])
@pytest.mark.parametrize("layout", list(SMALL))
@pytest.mark.parametrize("kind", KINDS)
def test_loo_epilogue_entrywise(ctx, opts, kind, layout, panel, resident):
    c = case(ctx, kind, layout)
    opts({"inverse_diag_panel": panel, "trsv_resident": resident})
    w, d = c.mat.solve_weights(c.r), c.mat.inverse_diag()
    mean, var, logp, total = c.mat.loo(c.r, c.y)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(logp)) and np.isfinite(total)
    assert np.array_equal(var, 1.0 / d), "var != 1 / d bit for bit: do lpgp_mat_loo and lpgp_mat_inverse_diag run the same launches?"
    m_ref, _, l_ref = fr.loo(w, d, c.y)
    step = np.abs(w.astype(LD) / d.astype(LD))
    em, im = worst((np.abs(mean.astype(LD) - m_ref) / (U * (2 * step + np.abs(m_ref)))).astype(np.float64))
    half_log, quad = np.abs(LD(0.5) * np.log(d.astype(LD))), LD(0.5) * w.astype(LD) ** 2 / d.astype(LD)
    err_l = np.abs(logp.astype(LD) - l_ref)
    el, il = worst((err_l / (U * ((LOG_ULPS + 2) * half_log + 5 * quad + 2 * HALF_LOG_2PI))).astype(np.float64))
    t_ref = np.sum(logp.astype(LD))
    et = float(abs(LD(total) - t_ref) / (SUM_ULPS * U * np.sum(np.abs(logp.astype(LD)))))
    print(f"\n[loo {kind} {layout} panel={panel} resident={resident}] mean {em:.3f} (row {im}), logp {el:.3f} (row {il}), total {et:.3f} of their bounds")
    assert em <= 1.0 + 1e-9, f"LOO mean row {im}: {em:.2f} x the bound of three roundings"
    assert el <= 1.0 + 1e-9, f"LOO log density row {il}: {el:.2f} x its bound"
    assert et <= 1.0, f"sum of the log densities over the logical rows: {et:.2f} x the bound of its reduction"


# ---- f: variance and std through the public interface --------------------------------------------------------------------
def posteriors(lp, blocks):
    """One posterior per appended block of the noise-"s" problem, built through the public interface."""
    cf = lp.randprocs.covfuncs
    X, noise = gram_points("s", sum(blocks))
    Y = np.random.default_rng(sum(blocks)).standard_normal(sum(blocks))
    u = lp.GaussianProcess(lp.functions.Zero((2,)), cf.Matern((2,), nu=2.5, lengthscales=0.3))
    out, lo = [], 0
    for nb in blocks:
        u = u.condition_on_observations(Y[lo:lo + nb], X[lo:lo + nb], b=lp.randvars.Normal(np.zeros(nb), noise[lo:lo + nb]))
        out.append(u)
        lo += nb
    return out


@pytest.mark.parametrize("panel", PANELS, ids=[f"panel{p}" for p in PANELS])
@pytest.mark.parametrize("layout", ["n300", "chain", "view"])
def test_public_loo_variance_componentwise(ctx, opts, layout, panel):
    import linpde_gp_amd as lp
    blocks, view = SMALL[layout]
    us = posteriors(lp, blocks)
    u = us[-1] if view is None else us[view - 1]          # (the earlier posterior, asked after the later blocks were appended)
    opts({"inverse_diag_panel": panel})
    got = u.leave_one_out()
    mat = u._state.mat
    assert mat.ctx.get_option("inverse_diag_panel") == panel and mat.n == got.var.size == sum(blocks[:view])
    L = mat.todense("factor")
    ref = fr.inverse_diag(fr.inverse(L))
    W = scipy.linalg.solve_triangular(L, np.eye(L.shape[0]), lower=True)
    d_lap = np.sum(W * W, axis=0)
    span = float(np.log10(float(ref.max() / ref.min())))
    assert span >= 8.0
    for name, dev, lap, want in (("var", got.var, 1.0 / d_lap, LD(1) / ref), ("std", got.std, np.sqrt(1.0 / d_lap), np.sqrt(LD(1) / ref))):
        e, e_ref = fr.relative_error(dev, want), fr.relative_error(lap, want)
        print(f"\n[public loo {name} {layout} panel={panel}] relative error {e / U:.1f} u (LAPACK {e_ref / U:.1f} u): ratio {e / e_ref:.3f}; over {span:.1f} decades")
        assert e <= RATIO_D * e_ref, f"LOO {name}: {e / U:.1f} u = {e / e_ref:.2f} x LAPACK's {e_ref / U:.1f} u"


# ---- g: several rows per thread (capped launches), the exact case, the padding status --------------------------------------
CAPPED = ["n700", "chain"]          # 768 padded rows each: k = 3 rows per thread with one workgroup, 2 with two


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("layout", CAPPED)
@pytest.mark.parametrize("kind", KINDS)
def test_evidence_terms_several_rows_per_thread(ctx, kind, layout, cap):
    import _hooks
    c = case(ctx, kind, layout)
    pn = c.mat.padded_n
    k = fr.reduction_depth(pn, cap)
    assert pn == 768 and k == {1: 3, 2: 2}[cap] and fr.sum_ulps(1) == SUM_ULPS and fr.log_ulps(1, LOG_ULPS) == LOG_ULPS
    zp = _hooks.solve_vec_fwd(ctx, c.mat, c.r)
    q, logdet = _hooks.evidence(ctx, c.mat, c.r, cap)
    assert _hooks.evidence(ctx, c.mat, c.r, 0) == c.mat.evidence(c.r), "the hook without a cap is not the public call"
    assert _hooks.evidence(ctx, c.mat, c.r, cap) == (q, logdet)
    q_ref = np.sum(zp.astype(LD) ** 2)
    eq = float(abs(LD(q) - q_ref) / (fr.sum_ulps(k) * U * q_ref))
    ld_ref, scale = fr.logdet(c.diag)
    el = float(abs(LD(logdet) - ld_ref) / (U * scale))
    print(f"\n[evidence {kind} {layout} cap={cap} k={k}] q {q:.17e}: {eq:.3f} of the bound; log det {logdet:.17e}: {el:.3f} u 2 sum |log L_ii| "
          f"(bar {fr.log_ulps(k, LOG_ULPS):.0f})")
    assert eq <= 1.0, f"r^T G^-1 r is {eq:.2f} x the bound of its reduction at {k} rows per thread"
    assert el <= fr.log_ulps(k, LOG_ULPS), f"log det is {el:.2f} u 2 sum |log L_ii| from 2 sum log L_ii at {k} rows per thread"


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("layout", CAPPED)
@pytest.mark.parametrize("kind", KINDS)
def test_loo_several_rows_per_thread(ctx, kind, layout, cap):
    import _hooks
    c = case(ctx, kind, layout)
    k = fr.reduction_depth(c.mat.padded_n, cap)
    base = c.mat.loo(c.r, c.y)
    free = _hooks.loo(ctx, c.mat, c.r, c.y, 0)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(base, free)), "the hook without a cap is not the public call"
    mean, var, logp, total = _hooks.loo(ctx, c.mat, c.r, c.y, cap)
    for name, a, b in (("mean", mean, base[0]), ("var", var, base[1]), ("logp", logp, base[2])):
        assert a.tobytes() == b.tobytes(), f"LOO {name} per row depends on the grid"
    t_ref = np.sum(logp.astype(LD))
    et = float(abs(LD(total) - t_ref) / (fr.sum_ulps(k) * U * np.sum(np.abs(logp.astype(LD)))))
    print(f"\n[loo {kind} {layout} cap={cap} k={k}] total {total:.17e}: {et:.3f} of the bound")
    assert np.isfinite(total) and et <= 1.0, f"sum of the log densities: {et:.2f} x the bound of its reduction at {k} rows per thread"


def test_evidence_exact_on_the_identity_factor(ctx):
    import _exact_operands as ex
    import _hooks
    mat = ex.identity_factored(ctx, CHAIN)
    assert mat.padded_n == 768
    r = np.random.default_rng(621).integers(-8, 9, mat.n)
    want = (float(np.sum(r * r)), 0.0)
    rf = r.astype(np.float64)
    zp = _hooks.solve_vec_fwd(ctx, mat, rf)
    assert np.array_equal(zp[ex.logical_mask(CHAIN)], rf), "a solve against the identity factor does not return r exactly"
    for cap in (1, 2, 0):
        got = _hooks.evidence(ctx, mat, rf, cap)
        print(f"\n[evidence exact cap={cap}] {got!r}, want {want!r}")
        assert got == want and not np.signbit(got[1]), (cap, got, want)
    assert mat.evidence(rf) == want


def test_padding_row_status(ctx):
    import _exact_operands as ex
    import _hooks
    from linpde_gp_amd._lib import LpgpError
    mat = ex.identity_factored(ctx, CHAIN)
    mask = ex.logical_mask(CHAIN)
    r = np.random.default_rng(622).integers(-8, 9, mat.n).astype(np.float64)
    good = _hooks.mat_raw(ctx, mat).copy()
    before = {cap: _hooks.evidence(ctx, mat, r, cap) for cap in (0, 1)}
    assert before[0] == mat.evidence(r)
    for row, cap in ((200, 0), (400, 1), (767, 1)):          # padding rows of the first trip, the second and the third
        assert not mask[row] and (cap == 0 or row // 256 == {400: 1, 767: 2}[row])
        bad = good.copy()
        bad[row, row] = 2.0
        _hooks.mat_raw(ctx, mat, bad)
        with pytest.raises(LpgpError, match="padding row of the factor"):
            _hooks.evidence(ctx, mat, r, cap)
        with pytest.raises(LpgpError, match="padding row of the factor"):
            mat.evidence(r)
        _hooks.mat_raw(ctx, mat, good)
        assert _hooks.evidence(ctx, mat, r, cap) == before[cap], "the call after the entry was restored returns other bits"
    assert mat.evidence(r) == before[0]
