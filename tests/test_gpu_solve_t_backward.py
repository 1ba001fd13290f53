"""The backward substitutions x = L^-T y -- the three pieces of device code behind the second half of every solve -- held to the
DEVICE'S OWN factor, each alone (the method of test_gpu_evidence_backward.py for the forward half, whose cases these are):
  trsv_bwd_resident_kernel (trsv.hip; trsv_resident = 1, the default) and trsv_bwd_head_kernel / trsv_bwd_step_kernel (potrf.hip;
  trsv_resident = 0) through the hook lpgp_test_solve_vec_bwd, which calls the functions solve_vec / solve_vec_resident call;
  trsm_lower_t_blocked (potrf.hip), the multi-column form behind lpgp_potrs, through the hook lpgp_test_trsm_lower_t.
L is `todense("factor")`; every residual is formed in long double (tests/_factor_reference.py: lower_tmv, backward_error_t, checked
against 50-digit mpmath in test_factor_reference.py).  The measure is the COMPONENTWISE backward error
max_i |y - L^T x|_i / (|L^T||x| + |y|)_i (0 / 0 counts 0, a nonzero residual over 0 fails), against the same measure of
scipy.linalg.solve_triangular(L, y, lower=True, trans="T") on the same L and y: a normwise measure of G x = b, which is all the
suite had for this half, does not see a small component of x that is wrong.

  a  single vector, both forms, the kinds and layouts of test_gpu_evidence_backward.py (its `Case`); two right-hand sides:
       "z"       the device's own forward half of the smooth residual (lpgp_test_solve_vec_fwd), so that x is the representer
                 weights the product computes: gathered to logical rows x must equal `solve_weights(r)` byte for byte;
       "normal"  a seeded standard normal vector.
     <= RATIO_X[form] x solve_triangular's.  With zeros in the padding of y: every padding entry of x exactly 0.0, two runs the same
     bytes (the resident kernel hands over through sentinel polling: a difference is a race).  With the constant PAD in the
     padding of y: the logical rows of x equal the zero-padding run entry for entry and the padding of x equals the padding of y bit for
     bit (the padded part of every diagonal tile and of its inverse is the identity, the couplings are exact zeros).
  b  multi-column: m = 9, 128, 129, 300 columns (one, one, two, three column tiles) x nb = 128 (no inner panel update) and 512 (the
     outer update from 700 rows on, three times at 1600).  Right-hand sides as a gain solve has them: even columns V = L^-1 k(X, x_j)
     (host LAPACK) for prediction points x_j near observation points, odd columns standard normal.  Sampled columns: one of every
     16, the first, the last, both sides of every 128-column boundary; <= RATIO_M x solve_triangular's over the same sample.  Columns
     beyond m enter as zeros and come back exactly zero, padding rows exactly zero, two runs the same bytes.
  c  the public entry points beyond one column tile: `potrs(B)` with 129 and 300 right-hand sides, normwise against cho_solve on
     the device-assembled Gram at RATIO_SOLVE of test_gpu_potrf_backward.py; `condition_normal_on_observations` with a gain of
     200 columns against the dense formula at the tolerances of test_gpu_parity.py.

Measured on the MI355X (every figure is printed by its test; MEASUREMENTS.md has the table):
  RATIO_X   largest device / LAPACK ratio: resident 0.78 (b, view, rhs z: 1.49 u against 1.93 u), per tile row 0.75 (m, 128 rows, rhs
            normal); every one of the 104 cases is BELOW solve_triangular's error, from 1600 rows on below 0.5 (s, 4700 rows: 3.2 u
            against LAPACK's 26.5 u).  The bars are 2 x 0.75 and 2 x 0.78 rounded down.
  RATIO_M   largest ratio 2.25 (h, 1600 rows, m = 9, nb = 512: 19.5 u against 8.7 u); nb = 128: 2.20 (s, chain, m = 300); per kind
            m 1.1 - 1.6, b 0.6 - 1.8, s 1.0 - 2.2, h 0.5 - 2.3.  The three GEMM products of a tile step round more often than the
            single-vector kernels do.
  c: potrs 0.35 - 0.46 of cho_solve's normwise backward error.  The padding checks of a hold as written in both forms on all 104 cases.
Defect runs (recorded, not tests; in-bounds wrong arithmetic):
  no refinement step in the resident solves (LPGP_TRSV_FLAGS=1, fresh process): 38 of the 52 resident cases of a fail (b 16 of 16, s 14
    of 16, h 4 of 4, m 4 of 16), ratios up to 9.2 (h, 700 rows, rhs z; 6.8 with rhs normal) where the unchanged kernel has at most 0.78;
    the 52 per-tile cases, which the flag does not reach, pass.  Both right-hand sides expose it on "h".
  trsm_lower_t_blocked without its second and third product (one scratch build): 75 of the 128 cases of b fail (h 41 of 56, b 32 of
    56, s 2 of 8, m 0 of 8), ratios up to 50 (h and b, 100 rows); the four normwise potrs cases of c PASS on that build (0.34 - 0.76 of
    cho_solve's): the measure the suite had does not see this defect."""
import numpy as np
import pytest
import scipy.linalg

import _factor_reference as fr
from _backward import restored, solve_backward_error
from test_gpu_evidence_backward import LARGE, SMALL, Case

pytestmark = pytest.mark.gpu

U = fr.U
RATIO_X = {1: 1.5, 0: 1.5}     # a: backward error of x <= RATIO_X[trsv_resident] x solve_triangular's  (<= twice the largest measured)
RATIO_M = 4.5                  # b: the same for the sampled columns of the multi-column form             (<= twice the largest measured)
PAD = 0.75                     # a: the nonzero constant in the padding of y

KINDS = ["m", "b", "s"]
VEC_CASES = [(k, la) for k in KINDS for la in list(SMALL) + list(LARGE)] + [("h", "n700"), ("h", "n1600")]
MS = [9, 128, 129, 300]
NBS = [128, 512]
MAT_LAYOUTS = list(SMALL) + ["n1600"]
MAT_CASES = [(k, la) for k in ("b", "h") for la in MAT_LAYOUTS] + [("m", "chain"), ("s", "chain")]


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    yield _engine.default_context()
    _cases.clear()                  # (the matrices go while the library is still loaded)


@pytest.fixture
def opts(ctx):
    with restored(ctx, ("trsv_resident", "nb")) as apply:
        yield apply


_cases = {}


def case(ctx, kind, layout):
    """The cases of at most 700 rows are kept for the whole module; of the larger ones only the last."""
    key = (kind, layout)
    if key not in _cases:
        for k in [k for k in _cases if k[1] in LARGE]:
            del _cases[k]
        _cases[key] = Case(ctx, kind, *(SMALL.get(layout) or LARGE[layout]))
    return _cases[key]


def padding(c):
    pad = np.ones(c.mat.padded_n, dtype=bool)
    pad[c.rows] = False
    return pad


def solve_t(L, y):
    return scipy.linalg.solve_triangular(L, y, lower=True, trans="T")


# ---- a: the single vector ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rhs", ["z", "normal"])
@pytest.mark.parametrize("resident", [1, 0], ids=["resident", "per_tile"])
@pytest.mark.parametrize("kind,layout", VEC_CASES)
def test_backward_solve_backward_error(ctx, opts, kind, layout, resident, rhs):
    import _hooks
    c = case(ctx, kind, layout)
    opts({"trsv_resident": resident})
    pad = padding(c)
    if rhs == "z":
        y = _hooks.solve_vec_fwd(ctx, c.mat, c.r)
        assert np.all(y[pad] == 0.0)
    else:
        y = np.zeros(c.mat.padded_n)
        y[c.rows] = c.once("normal", lambda: np.random.default_rng(3 * c.n + 2).standard_normal(c.n))
    x = _hooks.solve_vec_bwd(ctx, c.mat, y)
    assert x.shape == y.shape and np.all(np.isfinite(x))
    assert np.all(x[pad] == 0.0), "a padding entry of x is not exactly 0.0"
    again = _hooks.solve_vec_bwd(ctx, c.mat, y)
    assert x.tobytes() == again.tobytes(), "two runs of one form differ: no atomics in these solves, a difference is a race"
    if rhs == "z":
        w = c.mat.solve_weights(c.r)
        assert w.tobytes() == np.ascontiguousarray(x[c.rows]).tobytes(), "the two hooks chained are not the path of solve_weights"
    be = fr.backward_error_t(c.L, x[c.rows], y[c.rows])
    be_ref = c.once(("xt", rhs, resident if rhs == "z" else None), lambda: fr.backward_error_t(c.L, solve_t(c.L, y[c.rows]), y[c.rows]))
    print(f"\n[x {kind} {layout} resident={resident} rhs={rhs}] backward error {be / U:.2f} u (solve_triangular {be_ref / U:.2f} u): ratio {be / be_ref:.3f}")
    # a nonzero constant in the padding of y passes through to the padding of x and touches no logical row
    yp = y.copy()
    yp[pad] = PAD
    xp = _hooks.solve_vec_bwd(ctx, c.mat, yp)
    assert np.array_equal(xp[c.rows], x[c.rows]), "the padding of y reaches a logical row of x"
    assert xp[pad].tobytes() == yp[pad].tobytes(), "the padding of x is not the padding of y bit for bit"
    assert be <= RATIO_X[resident] * be_ref, f"backward error of x {be / U:.2f} u = {be / be_ref:.2f} x solve_triangular's {be_ref / U:.2f} u"


# ---- b: the multi-column form -----------------------------------------------------------------------------------------------
def columns(m):
    """One column of every 16, the first, the last, both sides of every 128-column boundary (test_gpu_predict_backward.py)."""
    rng = np.random.default_rng(m + 1)
    cols = {0, m - 1} | {b - 1 for b in range(128, m, 128)} | set(range(128, m, 128))
    cols |= {g + int(rng.integers(min(16, m - g))) for g in range(0, m, 16)}
    return np.array(sorted(cols))


def matern52_cross(X, Xt):
    r = np.sqrt(5.0) * np.sqrt(np.sum((X[:, None, :] - Xt[None, :, :]) ** 2, axis=-1)) / 0.3
    return (1 + r + r * r / 3) * np.exp(-r)


def block(c, m):
    """(Y in the padded layout with m_pad columns, the sampled columns, LAPACK's backward error on them), made once per case."""
    def make():
        rng = np.random.default_rng(1000 * c.n + m)
        X = c.ap.X[:c.n]
        Xt = X[rng.integers(c.n, size=m)] + 0.02 * rng.standard_normal((m, 2))
        Yl = scipy.linalg.solve_triangular(c.L, matern52_cross(X, Xt), lower=True)
        Yl[:, 1::2] = rng.standard_normal((c.n, m))[:, 1::2]
        Y = np.zeros((c.mat.padded_n, -(-m // 128) * 128), order="F")
        Y[c.rows, :m] = Yl
        cols = columns(m)
        ref = fr.backward_error_t(c.L, solve_t(c.L, Yl[:, cols]), Yl[:, cols])
        return Y, cols, ref
    return c.once(("Y", m), make)


@pytest.mark.parametrize("nb", NBS, ids=[f"nb{v}" for v in NBS])
@pytest.mark.parametrize("m", MS, ids=[f"m{v}" for v in MS])
@pytest.mark.parametrize("kind,layout", MAT_CASES)
def test_multi_column_backward_error(ctx, opts, kind, layout, m, nb):
    import _hooks
    c = case(ctx, kind, layout)
    Y, cols, ref = block(c, m)
    opts({"nb": nb})
    X = _hooks.trsm_lower_t(ctx, c.mat, Y)
    assert X.shape == Y.shape and np.all(np.isfinite(X))
    assert np.all(X[:, m:] == 0.0), "a column beyond m is not exactly zero"
    assert np.all(X[padding(c)] == 0.0), "a padding row of X is not exactly zero"
    again = _hooks.trsm_lower_t(ctx, c.mat, Y)
    assert X.tobytes(order="F") == again.tobytes(order="F"), "two runs differ: no atomics in this solve, a difference is a race"
    e = fr.backward_error_t(c.L, X[np.ix_(c.rows, cols)], Y[np.ix_(c.rows, cols)])
    j = int(np.argmax(e))
    be, be_ref = float(e[j]), float(np.max(ref))
    print(f"\n[X {kind} {layout} m={m} nb={nb}] backward error {be / U:.2f} u at column {cols[j]} (solve_triangular {be_ref / U:.2f} u, "
          f"there {ref[j] / U:.2f} u): ratio {be / be_ref:.3f}")
    assert be <= RATIO_M * be_ref, f"column {cols[j]}: backward error {be / U:.2f} u = {be / be_ref:.2f} x solve_triangular's {be_ref / U:.2f} u"


# ---- c: the public entry points beyond one column tile ---------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [129, 300])
@pytest.mark.parametrize("layout", ["chain", "n700"])
def test_potrs_beyond_one_column_tile(ctx, layout, nrhs):
    from test_gpu_potrf_backward import RATIO_SOLVE, appended_matrix, factor_appended, lapack
    blocks = SMALL[layout][0]
    n = sum(blocks)
    A = appended_matrix("b", n, blocks)              # the device-assembled Gram, read back before any factorisation
    mat = factor_appended(ctx, "b", n, blocks).mat
    B = np.random.default_rng(n + nrhs).standard_normal((n, nrhs))
    x = mat.potrs(B)
    assert x.shape == B.shape and np.all(np.isfinite(x))
    be = solve_backward_error(A, x, B)
    be_ref = solve_backward_error(A, scipy.linalg.cho_solve((lapack(A)[0], True), B), B)
    print(f"\n[potrs {layout} nrhs={nrhs}] backward error {be:.3e} (cho_solve {be_ref:.3e}): ratio {be / be_ref:.2f}")
    assert be <= RATIO_SOLVE * be_ref, f"{layout} nrhs={nrhs}: {be:.3e} vs cho_solve {be_ref:.3e}"


def test_condition_normal_on_observations_wide_gain():
    """The gain solve of `randvars/_normal.py` with 201 right-hand sides (two column tiles) on 140 observations (two tile rows),
    against the dense formula at the tolerances of test_gpu_parity.py::test_condition_normal_on_observations."""
    import linpde_gp_amd as lp
    rng = np.random.default_rng(47)
    n, m = 200, 140
    B = rng.standard_normal((n, n))
    prior = lp.randvars.Normal(rng.standard_normal(n), B @ B.T + n * np.eye(n))
    A = rng.standard_normal((m, n))
    Cn = rng.standard_normal((m, m))
    noise = lp.randvars.Normal(rng.standard_normal(m), Cn @ Cn.T + 0.1 * np.eye(m))
    y = rng.standard_normal(m)
    post = prior.condition_on_observations(y, noise, A)
    S = A @ prior.cov @ A.T + noise.cov
    K = np.linalg.solve(S, A @ prior.cov).T
    np.testing.assert_allclose(post.mean, prior.mean + K @ (y - A @ prior.mean - noise.mean), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(post.cov, prior.cov - K @ A @ prior.cov, rtol=1e-9, atol=1e-9)
