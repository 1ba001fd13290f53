"""The forward substitution of the prediction, V = L^{-1} K_Xx (`lpgp_predict`, `lpgp_potrf_predict`, `lpgp_trsm_lower`:
csrc/potrf.hip trsm_lower_blocked / trsm_lower_two_level / potrf_predict_blocked / ride_panel_now, solve_panel.h, chain.hip
panel_chain_v_kernel), its read-outs (api.hip col_reduce_kernel, col_reduce2_kernel) and the single right-hand side (trsv.hip),
against LAPACK-level accuracy over the options that select their branches.

Every reference is built on the device's own operands -- K0, the assembled cross-covariance read back before the solve; V, read
back after it; L, the device's factor -- so that the measures see the substitution and the read-outs alone:
  V     componentwise backward error per column, max_i |K0 - L V|_ij / (|L| |V| + |K0|)_ij with the residual in long double
        (0/0 counts 0, a nonzero residual over 0 fails), against LAPACK's dtrsm (scipy.linalg.solve_triangular) on the same L
        and K0.  Sampled columns: one of every 16 (a workgroup owns 16 or 32 columns: every workgroup is checked), the first and
        the last, both sides of the first 128-column tile boundary;
  var   against k_xx - sum_i V_ij^2, summed in long double over the LOGICAL rows (padded rows that are not exactly zero show
        here), at the a-priori bound of the kernel's summation order;
  mean  V^T z (the residual rides as column m) against K0^T L^{-T} L^{-1} r in long double, relative to the distance of the
        same formula in double with LAPACK; K0^T w (weights) against the long-double product at the kernel's bound;
  bits  two runs of one route give the same V bit for bit: the solves use no atomics, a difference is a race.
Observations: a Matern-5/2 on scattered points of [0, 0.5]^2 with a nugget of 1e-8 (the worst diagonal tile of L has cond >= 1e4, so that a
tile solve without its refinement step shows), one block or appended blocks (identity-padded tails, a panel grid shifted by the
appends); the first prediction points are observation points (variance ~ 0).  The c3 shape in small form and a derivative
read-out go through the package (`ConditionalGaussianProcess`).  Every route row asserts the route counters (`route_*` of
`lpgp_get_option`) that prove it reached its branch."""
import numpy as np
import pytest
import scipy.linalg

from _backward import EPS, LD, Appender, backward_error, gram_points, mtv, mv, restored

pytestmark = pytest.mark.gpu

# Bars, set from the first MI355X run (the largest measured value in brackets).  V's componentwise backward error is at most
# 1.2 x LAPACK's on the same L and K0 [1.21, the c3 shape's derivative read-out] and 0.0043 n eps in all; with the refinement step
# of the fused panel kernel dropped it is 2.9 - 880 x LAPACK's.  The read-outs stay inside their a-priori bounds [0.095 of the
# variance's]; the mean V^T z is [6.5] x LAPACK's distance from the long-double value (both are cond-bound); solve_weights'
# normwise backward error is [0.41] x cho_solve's; the factor appended behind an augmented ride [0.07] x LAPACK's.
RATIO = 2.5            # V: componentwise backward error <= RATIO x LAPACK's on the same L and K0
CEIL = 0.01            # ... and <= CEIL * n * eps
RATIO_MEAN = 16.0      # mean V^T z: distance from the long-double value <= RATIO_MEAN x LAPACK's + the summation bound
RATIO_SOLVE = 2.0      # solve_weights: normwise backward error <= RATIO_SOLVE x cho_solve's
RATIO_FACTOR, CEIL_FACTOR = 10.0, 0.5      # a factor (the bars of test_gpu_potrf_backward.py)

OPTIONS = ("lookahead", "fused_solve", "fused_ahead", "fused_ahead_min_us", "nb_solve", "nb_outer_solve", "nb_outer_solve_min_tiles",
           "solve_chain_us_tile", "chain_us_fixed", "ride_stream", "ride_same_stream_max_tiles", "ride_gate_pct", "ride_outer_rows",
           "ride_outer_min_tiles", "ride_vchain_max_wgs", "ride_occ3", "ride_max_tiles", "ride_aug", "gemm3", "trsv_resident")
ROUTES = ("ride_done", "ride_aug", "ride_b2b", "ride", "ride_vchain", "ride_two", "ride_outer", "solve_two_level", "solve_ahead",
          "solve_tiles")

T1, T5, T12, T36 = [100], [600], [1500], [4608]           # 1, 5, 12, 36 tile rows
APP = [300, 77, 1, 513, 1234]                              # 2 125 rows in 20 tile rows: tails of 84, 51, 127, 127, 46 padded rows


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


@pytest.fixture
def sched(ctx):
    with restored(ctx, OPTIONS) as apply:
        yield apply


def routes(ctx):
    return {k: ctx.get_option("route_" + k) for k in ROUTES}


def padded(nb):
    return -(-nb // 128) * 128


def padded_row(blocks, i):
    off = poff = 0
    for nb in blocks:
        if i < off + nb:
            return poff + i - off
        off, poff = off + nb, poff + padded(nb)
    raise IndexError(i)


def observation_points(n):
    """n scattered points in [0, 0.5]^2 and a nugget of 1e-8: with the lengthscale 0.3 the worst diagonal tile of L has
    cond >= 2e4 from 600 rows on."""
    X, noise = gram_points("b", n)
    return 0.5 * X, noise


def prediction_points(X, m):
    """m prediction points in [0, 0.5]^2; the first min(m, 8) are observation points (variance ~ 0)."""
    rng = np.random.default_rng(m)
    Xt = rng.uniform(0, 0.5, (m, 2))
    k = min(m, 8)
    Xt[:k] = X[rng.choice(X.shape[0], k, replace=False)]
    return Xt


class Case:
    """A fresh problem: observation blocks `blocks` (the first `factored` factored as they arrive; default all), m prediction
    points; K0 read back.  `capacity`: "room" (space for the augmented ride below the blocks), "tight" (none) or None."""

    def __init__(self, ctx, blocks, m, factored=None, capacity=None, spare=0):
        from linpde_gp_amd import _engine
        self.ctx, self.blocks, self.m, self.n = ctx, list(blocks), m, sum(blocks)
        pn = sum(padded(nb) for nb in blocks)
        cap = {None: None, "room": pn + padded(m + 1) + 128, "tight": pn}[capacity]
        X, noise = observation_points(self.n + spare)
        self.ap = Appender(ctx, X, noise, cap)
        for i, nb in enumerate(blocks):
            self.ap.add(nb)
            if factored is None or i < factored:
                assert self.ap.mat.potrf() == 0
        self.mat = self.ap.mat
        self.pts = _engine.Points(ctx, prediction_points(X[:self.n], m))
        self.rhs = self.cross()
        self.K0 = self.rhs.to_host()
        self.r = np.random.default_rng(self.n + 1).standard_normal(self.n)
        self.kxx = np.ones(m)                    # (unit variance)

    def cross(self, pts=None, m=None):
        from linpde_gp_amd import _engine
        rhs = _engine.Rhs(self.ctx, self.mat, m or self.m)
        for bi in range(len(self.blocks)):
            rhs.cross_assemble(self.ap.kd, self.ap.pts[bi], pts or self.pts, bi)
        return rhs

    def predict(self, kind):
        """kind "predict" (lpgp_predict, the residual riding as column m) or "ride" (lpgp_potrf_predict); the route counters'
        increments in `routes`."""
        self.mat.set_residual(self.r)
        before = routes(self.ctx)
        if kind == "predict":
            self.mean, self.var = self.rhs.predict(None, self.kxx)
        else:
            self.mean, self.var = self.rhs.potrf_predict(None, self.kxx)
            assert self.mat.check()[0] == 0
        after = routes(self.ctx)
        self.routes = {k: after[k] - before[k] for k in ROUTES}
        self.V = self.rhs.to_host()
        self.L = self.mat.todense("factor")
        return self


# ---- measures ------------------------------------------------------------------------------------------------------------
def columns(m):
    rng = np.random.default_rng(m + 1)
    cols = {0, m - 1, min(m, 128) - 1, min(m - 1, 128)}
    cols |= {g + int(rng.integers(min(16, m - g))) for g in range(0, m, 16)}
    return np.array(sorted(cols))


def lower_mv(L, X):
    """L @ X for lower-triangular L in long double (row slabs: only the columns left of the slab's end)."""
    XL = X.astype(LD)
    out = np.empty(X.shape, dtype=LD)
    for i in range(0, L.shape[0], 512):
        e = min(i + 512, L.shape[0])
        out[i:e] = L[i:e, :e].astype(LD) @ XL[:e]
    return out


def cw_error(L, K, V):
    """|K - L V| / (|L| |V| + |K|) entrywise (0/0 = 0)."""
    R = np.abs(K.astype(LD) - lower_mv(L, V)).astype(np.float64)
    D = np.abs(L) @ np.abs(V) + np.abs(K)
    zero = D == 0.0
    assert not np.any(R[zero] != 0.0), "a nonzero residual where |L||V| + |K0| is zero"
    return np.where(zero, 0.0, R / np.where(zero, 1.0, D))


def sum_bound(pn):
    """Relative error of col_reduce(2)_kernel's sums over pn rows: a thread chains 2 ceil(pn / 512) fused multiply-adds, then six
    shuffle levels and two over the workgroup's four waves, and the host forms k_xx - sum (+ slack)."""
    return (2 * (-(-pn // 512)) + 16) * EPS


def check_V(c, tag):
    n, m = c.K0.shape
    assert np.all(np.isfinite(c.V)), f"{tag}: V is not finite"
    cols = columns(m)
    K, V = c.K0[:, cols], c.V[:, cols]
    E = cw_error(c.L, K, V)
    rc = cols[::max(1, len(cols) // 16)]
    Kr = c.K0[:, rc]
    be_ref = float(np.max(cw_error(c.L, Kr, scipy.linalg.solve_triangular(c.L, Kr, lower=True))))
    be = float(E.max())
    i, j = np.unravel_index(int(np.argmax(E)), E.shape)
    where = f"tile row {padded_row(c.blocks, i) // 128} (row {i}), column {cols[j]}"
    ratio = be / max(be_ref, EPS)
    print(f"\n[V {tag}] backward error {be:.3e} (LAPACK {be_ref:.3e}): ratio {ratio:.2f}, {be / (n * EPS):.4f} n eps; worst at {where}")
    assert be <= RATIO * max(be_ref, EPS), f"{tag}: V backward error {be:.3e} = {ratio:.1f} x LAPACK's {be_ref:.3e}, worst at {where}"
    assert be <= CEIL * n * EPS, f"{tag}: V backward error {be:.3e} > {CEIL} n eps, worst at {where}"


def check_var(c, tag):
    s = np.sum(c.V.astype(LD) ** 2, axis=0)
    err = np.abs(c.var.astype(LD) - (c.kxx.astype(LD) - s)).astype(np.float64)
    bound = sum_bound(c.mat.padded_n) * s.astype(np.float64) + EPS * np.abs(c.kxx)
    j = int(np.argmax(err / bound))
    print(f"[var {tag}] worst |var - (k_xx - sum V^2)| = {err[j]:.3e}: {err[j] / bound[j]:.3f} of the bound (column {j})")
    assert np.all(err <= bound), f"{tag}: variance of column {j} off by {err[j]:.3e} = {err[j] / bound[j]:.3g} x the bound {bound[j]:.3e}"


def ld_solve(L, b, trans=False):
    """L x = b (trans: L^T x = b) in long double, by tiles of 128 rows."""
    n = L.shape[0]
    x = np.zeros(n, dtype=LD)
    for i0 in (range((n - 1) // 128 * 128, -1, -128) if trans else range(0, n, 128)):
        i1 = min(i0 + 128, n)
        Lb = L[i0:i1, i0:i1].astype(LD)
        if trans:
            rhs = b[i0:i1].astype(LD) - L[i1:, i0:i1].astype(LD).T @ x[i1:]
            for i in range(i1 - i0 - 1, -1, -1):
                x[i0 + i] = (rhs[i] - Lb[i + 1:, i] @ x[i0 + i + 1:i1]) / Lb[i, i]
        else:
            rhs = b[i0:i1].astype(LD) - L[i0:i1, :i0].astype(LD) @ x[:i0]
            for i in range(i1 - i0):
                x[i0 + i] = (rhs[i] - Lb[i, :i] @ x[i0:i0 + i]) / Lb[i, i]
    return x


def check_mean_z(c, tag):
    """mean = V^T z, z = L^{-1} r riding as column m, against K0^T L^{-T} L^{-1} r: two long-double substitutions on the device L."""
    y = ld_solve(c.L, c.r)
    ref = mtv(c.K0, ld_solve(c.L, y, trans=True)[:, None])[:, 0]
    yd = scipy.linalg.solve_triangular(c.L, c.r, lower=True)
    lap = c.K0.T @ scipy.linalg.solve_triangular(c.L, yd, lower=True, trans="T")
    d_dev = float(np.max(np.abs(c.mean.astype(LD) - ref)))
    d_lap = float(np.max(np.abs(lap.astype(LD) - ref)))
    floor = sum_bound(c.mat.padded_n) * float(np.max(np.abs(c.V).T @ np.abs(yd)))
    print(f"[mean {tag}] |V^T z - ref| = {d_dev:.3e} (LAPACK {d_lap:.3e}, summation bound {floor:.3e}): "
          f"ratio {d_dev / max(d_lap, floor):.2f}")
    assert d_dev <= RATIO_MEAN * d_lap + floor, f"{tag}: mean off by {d_dev:.3e}, LAPACK's formula by {d_lap:.3e}"


def check_case(c, tag, must, must_not):
    for key in must:
        assert c.routes[key] > 0, f"{tag}: route counter {key} did not count: the row no longer reaches its branch ({c.routes})"
    for key in must_not:
        assert c.routes[key] == 0, f"{tag}: route counter {key} counted {c.routes[key]} ({c.routes})"
    check_V(c, tag)
    check_var(c, tag)
    check_mean_z(c, tag)


# ---- route table ---------------------------------------------------------------------------------------------------------
# (id, kind, options, cases (blocks, m[, blocks factored before the call[, capacity]]), counters that must count / must not)
ROWS = [
    # the plain substitution (lpgp_predict)
    ("narrow", "predict", {}, [(T1, 1), (T5, 127), (T12, 128), (APP, 700), (T36, 1)], [],
     ["solve_ahead", "solve_tiles", "solve_two_level"]),
    ("wide_ahead", "predict", {"fused_ahead_min_us": 0}, [(T12, 1100), (T5, 2560)], ["solve_ahead"], ["solve_tiles"]),
    ("fused_ahead0_chain_bound", "predict", {"fused_ahead": 0, "solve_chain_us_tile": 1000000, "chain_us_fixed": 0}, [(T12, 1100)],
     [], ["solve_ahead", "solve_tiles"]),
    ("fused_ahead0_update_bound", "predict", {"fused_ahead": 0, "solve_chain_us_tile": 0, "chain_us_fixed": 0}, [(T12, 1100)],
     [], ["solve_ahead", "solve_tiles"]),
    ("fused_solve0_wide", "predict", {"fused_solve": 0}, [(T12, 1100), (APP, 127)], ["solve_tiles"], ["solve_ahead"]),
    ("nb_solve768", "predict", {"nb_solve": 768}, [(T12, 1100)], ["solve_tiles"], ["solve_ahead"]),
    ("lookahead0", "predict", {"lookahead": 0}, [(T12, 1100)], [], ["solve_ahead"]),
    ("two_level", "predict", {"nb_outer_solve": 1024, "nb_outer_solve_min_tiles": 16}, [(APP, 1100)], ["solve_two_level"], []),
    # the substitution riding inside the factorisation (lpgp_potrf_predict)
    ("ride_factored", "ride", {}, [(T12, 700)], ["ride_done"], ["ride", "ride_aug", "ride_b2b"]),
    ("ride_default", "ride", {}, [(T5, 127, 0), (T12, 1100, 0), (APP, 700, 3), (T1, 1, 0)], ["ride"], ["ride_aug", "ride_b2b"]),
    ("ride_two_halves", "ride", {"ride_stream": 1 + 8 * 4}, [(T12, 1100, 0)], ["ride", "ride_two"], []),
    ("ride_same_stream", "ride", {"ride_same_stream_max_tiles": 1000}, [(T12, 1100, 0)], ["ride"], ["ride_two"]),
    ("ride_gate0", "ride", {"ride_gate_pct": 0}, [(APP, 700, 2)], ["ride"], []),
    ("ride_gate30", "ride", {"ride_gate_pct": 30}, [(APP, 700, 2)], ["ride"], []),
    ("ride_gate100", "ride", {"ride_gate_pct": 100}, [(APP, 700, 2)], ["ride"], []),
    ("ride_two_level", "ride", {"ride_outer_rows": 1024, "ride_outer_min_tiles": 1}, [(APP, 1100, 2)], ["ride", "ride_outer"], []),
    ("ride_vchain", "ride", {"ride_vchain_max_wgs": 96}, [(T12, 700, 0)], ["ride", "ride_vchain"], []),
    ("ride_vchain0", "ride", {"ride_vchain_max_wgs": 0}, [(T12, 700, 0)], ["ride"], ["ride_vchain"]),
    ("ride_occ3_0", "ride", {"ride_occ3": 0, "gemm3": 64}, [(APP, 1100, 2)], ["ride"], []),
    ("ride_fused_solve0", "ride", {"fused_solve": 0}, [(T12, 700, 0)], ["ride"], ["ride_vchain"]),
    ("ride_back_to_back", "ride", {"ride_max_tiles": 4}, [(T12, 700, 0)], ["ride_b2b"], ["ride"]),
    ("ride_aug", "ride", {"ride_aug": 1}, [(T12, 700, 0, "room"), (APP, 1100, 3, "room")], ["ride_aug"], ["ride"]),
    ("ride_aug_no_room", "ride", {"ride_aug": 1}, [(T12, 700, 0, "tight")], ["ride"], ["ride_aug"]),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_route(ctx, sched, row):
    name, kind, opts, cases, must, must_not = row
    sched(opts)
    for k, case in enumerate(cases):
        blocks, m = case[0], case[1]
        args = (ctx, blocks, m, case[2] if len(case) > 2 else None, case[3] if len(case) > 3 else None)
        c = Case(*args).predict(kind)
        check_case(c, f"{name} n={c.n} ({len(blocks)} blocks) m={m}", must, must_not)
        if k == 0:
            # run-to-run bit identity: no atomics in these solves -- a difference is a race
            c2 = Case(*args).predict(kind)
            assert np.array_equal(c.V, c2.V) and np.array_equal(c.L, c2.L), f"{name}: two runs of the route differ"
            assert np.array_equal(c.mean, c2.mean) and np.array_equal(c.var, c2.var), f"{name}: two runs' read-outs differ"


def test_the_nugget_makes_the_diagonal_tiles_ill_conditioned(ctx):
    """Without cond(L_jj) >= 1e4 a tile solve that lost its refinement step would pass the bars."""
    c = Case(ctx, T12, 1).predict("predict")
    worst = max(np.linalg.cond(c.L[i:i + 128, i:i + 128]) for i in range(0, 1408, 128))
    print(f"\nworst diagonal tile of L: cond {worst:.2e}")
    assert worst >= 1e4


def test_augmented_ride_then_append(ctx, sched):
    """The augmented ride factors K_Xx^T as rows below the blocks, exactly where the next block goes: after it one more block is
    appended and factored, and the factor must be that of the device-assembled matrix (nothing of the scratch rows leaks)."""
    sched({"ride_aug": 1})
    extra = 300
    c = Case(ctx, APP, 1100, 3, "room", spare=extra).predict("ride")
    assert c.routes["ride_aug"] > 0
    check_V(c, "ride_aug before the append")
    c.ap.add(extra)
    assert c.mat.potrf() == 0
    twin = Appender(ctx, *observation_points(c.n + extra))
    for nb in APP + [extra]:
        twin.add(nb)
    G = twin.mat.todense("gram")
    L = c.mat.todense("factor")
    be, be_ref = backward_error(G, L), backward_error(G, np.linalg.cholesky(G))
    print(f"\n[append after ride_aug] factor backward error {be:.3e} (LAPACK {be_ref:.3e})")
    assert be <= RATIO_FACTOR * be_ref and be <= CEIL_FACTOR * G.shape[0] * EPS


@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("blocks", [T1, T5, T12, APP, T36], ids=["T1", "T5", "T12", "appended", "T36"])
def test_solve_weights_and_the_weights_mean(ctx, sched, resident, blocks):
    """trsv.hip: the normwise backward error of G w = r (solve_weights) against cho_solve's; then the mean K0^T w
    (col_reduce_kernel) against the long-double product of the device's own K0 and w."""
    sched({"trsv_resident": resident})
    c = Case(ctx, blocks, 127)
    twin = Appender(ctx, *observation_points(c.n))
    for nb in blocks:
        twin.add(nb)
    G = twin.mat.todense("gram")
    w = c.mat.solve_weights(c.r)
    nG = float(np.max(np.sum(np.abs(G), axis=1)))

    def nbe(x):
        return float(np.max(np.abs(mv(G, x[:, None].astype(LD))[:, 0] - c.r))) / (nG * np.max(np.abs(x)) + np.max(np.abs(c.r)))
    be, be_ref = nbe(w), nbe(scipy.linalg.cho_solve((np.linalg.cholesky(G), True), c.r))
    print(f"\n[solve_weights resident={resident} n={c.n}] backward error {be:.3e} (cho_solve {be_ref:.3e}): ratio {be / be_ref:.2f}")
    assert be <= RATIO_SOLVE * be_ref
    mean, _ = c.cross().predict(None, None, want_mean=True, want_var=False)
    ref = mtv(c.K0, w.astype(LD)[:, None])[:, 0]
    err = np.abs(mean.astype(LD) - ref).astype(np.float64)
    bound = sum_bound(c.mat.padded_n) * (np.abs(c.K0).T @ np.abs(w))
    assert np.all(err <= bound), f"K0^T w: worst {np.max(err / bound):.2f} of the bound"


def test_trsm_lower_inner_matmul(ctx):
    """`lpgp_trsm_lower` held to the bar of the substitution; `Rhs.inner` and `Rhs.matmul` against long-double products of the
    device's own V0, V1 and B at a gamma_k bound (m not a multiple of 128)."""
    from linpde_gp_amd import _engine
    c = Case(ctx, APP, 200)
    V0 = c.cross()
    V0.trsm_lower()
    c.V, c.L = V0.to_host(), c.mat.todense("factor")
    check_V(c, "trsm_lower")
    V1 = c.cross(_engine.Points(ctx, prediction_points(c.ap.X, 127)[::-1].copy()), 127)
    V1.trsm_lower()
    V1h = V1.to_host()
    pn = c.mat.padded_n
    G = V0.inner(V1)
    err = np.abs(G.astype(LD) - mtv(c.V, V1h.astype(LD))).astype(np.float64)
    bound = pn * EPS / (1 - pn * EPS) * (np.abs(c.V).T @ np.abs(V1h))
    assert np.all(err <= bound), f"inner: worst {np.max(err / bound):.2f} of the bound"
    B = np.random.default_rng(5).standard_normal((200, 77))
    W = V0.matmul(B).to_host()
    err = np.abs(W.astype(LD) - mv(c.V, B.astype(LD))).astype(np.float64)
    k = 256
    bound = k * EPS / (1 - k * EPS) * (np.abs(c.V) @ np.abs(B))
    assert np.all(err <= bound), f"matmul: worst {np.max(err / bound):.2f} of the bound"


@pytest.mark.parametrize("deriv", [False, True], ids=["values", "derivative"])
def test_c3_shape(ctx, deriv):
    """Four boundary value blocks with a nugget and a Laplacian block (17 tile rows; rows that differ in scale by 10^2-10^3: an
    absolute threshold inside the solve shows in the componentwise measure), built through the package; the read-out of the
    values or of a derivative."""
    from linpde_gp_amd import _engine, problems, randvars
    from linpde_gp_amd.randprocs._gaussian_process import ConditionalGaussianProcess
    wl = problems.poisson_2d(n_side=40, n_bdry=40, m_side=24)
    u = problems.build_prior(wl)
    for o in wl.observations:
        X, Y = o.X_as_given()
        b = None if o.noise_var is None else randvars.Normal(np.zeros(Y.shape), np.full(o.X.shape[0], o.noise_var))
        u = u.condition_on_observations(Y, X=X, L=problems.operator_of(o.op, wl.d), b=b)
    u._check_current()
    v = ConditionalGaussianProcess(prior=u._prior, blocks=u._blocks, state=u._state, representer_weights=None,
                                   test_coeffs={(1, 0): 1.0}) if deriv else u
    c = Case.__new__(Case)
    c.mat, c.blocks = u._state.mat, list(u._state.mat.block_sizes)
    rhs = v._cross(_engine.Points(ctx, wl.Xtest))
    c.K0 = rhs.to_host()
    c.n, c.m = c.K0.shape
    u._ensure_residual()
    c.r = u._residual()
    c.kxx = np.full(c.m, v._prior_diag())
    c.mean, c.var = rhs.predict(None, c.kxx)
    c.V, c.L = rhs.to_host(), c.mat.todense("factor")
    assert c.mat.padded_n == 17 * 128
    tag = f"c3 shape {'derivative' if deriv else 'values'} n={c.n} m={c.m}"
    check_V(c, tag)
    check_var(c, tag)
    check_mean_z(c, tag)
