"""Hyperparameter gradients of the log marginal likelihood (GPML eq. 5.9) on the device: the derivative descriptor
(`lpgp_kdesc.dlog_lengthscale`, csrc/lower.cpp), the dense inverse (`lpgp_mat_inverse`), the streaming contraction
(`lpgp_mat_evidence_grad`, csrc/evidence_grad.hip) and `ConditionalGaussianProcess.log_marginal_likelihood_gradient()`.

References.  Kernel entries: the univariate factors differentiated by SymPy (in t = x - x' and in the lengthscale) and evaluated
in 50-digit mpmath, in the style of tests/test_oracle_kernels.py; bar: the project's entry bar, 4e-15 of the block maximum.
Inverse and gradient: NumPy / LAPACK on the oracle's Gram matrix, judged by the rule of tests/test_gpu_random.py -- the device
may be 4 x as far from a long-double-refined (or 50-digit) evaluation as LAPACK itself is (gradient: or 1e-12 relative).
Contraction alone: `math.fsum` of the logical terms; bar n eps sum |terms|."""
import ctypes as C
import functools
import math

import mpmath
import numpy as np
import pytest
import scipy.linalg
import sympy as sp

import _hooks
from oracle import covfuncs as ocf
from oracle import gp as ogp
from oracle import polynomials

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
ENTRY_RTOL = 4e-15
DPS = 50


@pytest.fixture(scope="module")
def lp():
    import linpde_gp_amd
    return linpde_gp_amd


@pytest.fixture(scope="module")
def ctx(lp):
    from linpde_gp_amd import _engine
    return _engine.default_context()


# ---- 50-digit reference of the (differentiated) univariate factors -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _factor_fn(family, p, n, dlog):
    """mpmath functions (t > 0 branch, t < 0 branch) of d^n/dt^n k(t; l), t = x - x' -- l d/dl of it if `dlog`."""
    t, l = sp.symbols("t l", real=True)
    out = []
    for s in ((t,) if family == "expquad" else (t, -t)):
        if family == "expquad":
            k = sp.exp(-s ** 2 / (2 * l ** 2))
        else:
            a = sp.sqrt(2 * p + 1) / l
            c = polynomials.matern_half_integer_coefficients(p)
            k = sum(sp.Rational(ck.numerator, ck.denominator) * (a * s) ** i for i, ck in enumerate(c)) * sp.exp(-a * s)
        e = sp.diff(k, t, n) if n else k
        if dlog:
            e = l * sp.diff(e, l)
        out.append(sp.lambdify((t, l), e, "mpmath"))
    return out[0], out[-1]


_FACTOR_BLOCKS = {}


def _factor_block(factor, n0, n1, dlog, x0, x1):
    """(len(x0), len(x1)) object array of mpf: d^n0/dx^n0 d^n1/dx'^n1 of the factor (l d/dl of it if dlog) at (x0_i, x1_j)."""
    family = factor[0]
    p, ell = (int(factor[1] - 0.5), factor[2]) if family == "matern" else (0, factor[1])
    key = (factor, n0, n1, bool(dlog), x0.tobytes(), x1.tobytes())
    hit = _FACTOR_BLOCKS.get(key)
    if hit is not None:
        return hit
    f_pos, f_neg = _factor_fn(family, p, n0 + n1, bool(dlog))
    lm = mpmath.mpf(float(ell))
    sign = -1 if n1 & 1 else 1
    same = x0.shape == x1.shape and np.array_equal(x0, x1)
    flip = -1 if (n0 + n1) & 1 else 1                  # k is even in t: its n-th derivative has the parity of n
    out = np.empty((len(x0), len(x1)), dtype=object)
    for i, a in enumerate(x0):
        am = mpmath.mpf(float(a))
        for j, b in enumerate(x1):
            if same and j > i:
                continue
            tm = am - mpmath.mpf(float(b))
            out[i, j] = sign * (f_pos if tm >= 0 else f_neg)(tm, lm)       # (t = 0: the derivative is continuous for n <= 2p, either branch)
            if same and j < i:
                out[j, i] = flip * out[i, j]
    if len(_FACTOR_BLOCKS) >= 64:
        _FACTOR_BLOCKS.clear()
    _FACTOR_BLOCKS[key] = out
    return out


def ref_block_mp(kernel, L0, L1, X0, X1, group=None, dlog=None):
    """Object array of mpf: (L0 k L1)(X0, X1) for the oracle's kernel description [(scale, [factor, ...]), ...]; `group`: that summand
    alone; `dlog` = j: its derivative by log lengthscale j."""
    with mpmath.workdps(DPS):
        total = None
        for g, (scale, factors) in enumerate(kernel):
            if group is not None and g != group:
                continue
            for a, ca in L0.items():
                for b, cb in L1.items():
                    term = mpmath.mpf(float(scale)) * mpmath.mpf(float(ca)) * mpmath.mpf(float(cb))
                    blk = None
                    for dd, f in enumerate(factors):
                        fb = _factor_block(f, a[dd], b[dd], dlog == dd, X0[:, dd], X1[:, dd])
                        blk = fb if blk is None else blk * fb
                    total = term * blk if total is None else total + term * blk
        return total


def ref_block(*args, **kw):
    return ref_block_mp(*args, **kw).astype(np.double)


def _device_groups(lp, kernel):
    cf = lp.randprocs.covfuncs
    summands = []
    for scale, factors in kernel:
        fs = [cf.Matern((), nu=f[1], lengthscales=f[2]) if f[0] == "matern" else cf.ExpQuad((), lengthscales=f[1]) for f in factors]
        summands.append(scale * cf.TensorProduct(*fs))
    k = summands[0]
    for s in summands[1:]:
        k = k + s
    return k


def _lower(lp, kernel, L0, L1, group=None, dlog=None):
    cf = lp.randprocs.covfuncs
    groups = cf.DifferentiatedCovarianceFunction(_device_groups(lp, kernel), L0, L1).lower()
    if group is not None:
        groups = [groups[group]]
    if dlog is not None:
        groups = [dict(g, dlog_lengthscale=dlog + 1) for g in groups]
    return groups


def _ops(d):
    ident = {(0,) * d: 1.0}
    first = {tuple(int(i == 0) for i in range(d)): 1.0}
    lap = {tuple(2 * int(i == j) for i in range(d)): 1.0 for j in range(d)}
    return {"id x id": (ident, ident), "d x id": (first, ident), "id x d": (ident, first), "lap x id": (lap, ident), "id x lap": (ident, lap)}


ENTRY_KERNELS = {
    "matern32": [(1.0, [("matern", 1.5, 0.7)])],
    "matern52": [(1.3, [("matern", 2.5, 0.45)])],
    "expquad": [(0.8, [("expquad", 0.35)])],
    "matern52 x expquad": [(2.0, [("matern", 2.5, 0.8), ("expquad", 0.5)])],
    "matern32 x matern52": [(1.0, [("matern", 1.5, 1.1), ("matern", 2.5, 0.6)])],
}


@pytest.mark.parametrize("name", list(ENTRY_KERNELS))
def test_derivative_entries_against_sympy_mpmath(lp, ctx, name):
    """Dense blocks of flagged descriptors (`lpgp_kernel_matrix`) against the SymPy-differentiated kernels in 50-digit mpmath:
    40 x 37 seeded points with coinciding pairs; identity, first derivative and Laplacian on either side; every lengthscale."""
    from linpde_gp_amd import _engine
    kernel = ENTRY_KERNELS[name]
    d = len(kernel[0][1])
    rng = np.random.default_rng(20261017 + d)
    X0, X1 = rng.uniform(-1, 1, (40, d)), rng.uniform(-1, 1, (37, d))
    X1[:6] = X0[:6]                                                    # coinciding pairs
    X1[6, 0] = X0[6, 0]                                                # ... and one that coincides in the first coordinate only
    P0, P1 = _engine.Points(ctx, X0), _engine.Points(ctx, X1)
    worst = 0.0
    for op, (L0, L1) in _ops(d).items():
        for j in range(d):
            got = _engine.kernel_matrix(ctx, _lower(lp, kernel, L0, L1, dlog=j), P0, P1)
            ref = ref_block(kernel, L0, L1, X0, X1, dlog=j)
            err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
            worst = max(worst, err)
            print(f"{name} [{op}] d/dlog l_{j}: {err:.2e} of the block maximum")
            assert err <= ENTRY_RTOL, (name, op, j, err)
    print(f"{name}: worst {worst:.2e}")


def test_flagged_specialised_assembly_is_bit_identical(lp, ctx):
    """A flagged block through `assemble_fast_kernel` (degrees as template parameters) and through the generic `assemble_kernel`
    (option asm_fast = 0): the same arithmetic, identical blocks.  A Matern-9/2 factor rises to degree 5 -- six coefficients, outside
    the templates: the generic kernel either way, and the same numbers as a Richardson difference of the plain kernel."""
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(12)
    cases = []
    for kernel in (ENTRY_KERNELS["matern32"], ENTRY_KERNELS["matern52"], ENTRY_KERNELS["expquad"], ENTRY_KERNELS["matern52 x expquad"],
                   [(1.0, [("matern", 4.5, 0.9)])]):
        d = len(kernel[0][1])
        X0, X1 = rng.uniform(-1, 1, (150, d)), rng.uniform(-1, 1, (77, d))
        for L0, L1 in list(_ops(d).values())[:4]:
            for j in range(d):
                cases.append((_lower(lp, kernel, L0, L1, dlog=j), X0, X1))
    try:
        for groups, X0, X1 in cases:
            P0, P1 = _engine.Points(ctx, X0), _engine.Points(ctx, X1)
            ctx.set_option("asm_fast", 0)
            ref = _engine.kernel_matrix(ctx, groups, P0, P1)
            ctx.set_option("asm_fast", 1)
            got = _engine.kernel_matrix(ctx, groups, P0, P1)
            assert np.all(np.isfinite(ref))
            np.testing.assert_array_equal(got, ref)
    finally:
        ctx.set_option("asm_fast", 1)
    # the degree-5 factor against a difference quotient of the plain kernel
    kernel = lambda l: [(1.0, [("matern", 4.5, l)])]
    ident = {(0,): 1.0}
    X0, X1 = rng.uniform(-1, 1, (150, 1)), rng.uniform(-1, 1, (77, 1))
    P0, P1 = _engine.Points(ctx, X0), _engine.Points(ctx, X1)
    got = _engine.kernel_matrix(ctx, _lower(lp, kernel(0.9), ident, ident, dlog=0), P0, P1)
    f = lambda t: ocf.LkL(kernel(0.9 * math.exp(t)), ident, ident, X0, X1)
    h = 2e-2
    fd = (4 * (f(h / 2) - f(-h / 2)) / h - (f(h) - f(-h)) / (2 * h)) / 3
    assert np.max(np.abs(got - fd)) <= 1e-7 * np.max(np.abs(fd))


def test_grid_block_of_a_flagged_descriptor(lp, ctx):
    """A 12 x 11 tensor-grid block: `lpgp_kron_fits` refuses a flagged descriptor (the 1-D factor matrices are built from plain
    factors), `GramMatrix.assemble` then assembles the grid entry-wise -- the same entries as the flattened grid without its factors,
    4e-15 of the block maximum -- and `lpgp_gram_assemble_grid` itself refuses instead of assembling the plain kernel."""
    from linpde_gp_amd import _engine, _lib
    kernel = ENTRY_KERNELS["matern52 x expquad"]
    f0, f1 = np.linspace(-1, 1, 12), np.linspace(-0.5, 0.7, 11)
    X = np.stack(np.meshgrid(f0, f1, indexing="ij"), axis=-1).reshape(-1, 2)
    ident = {(0, 0): 1.0}
    lap = {(2, 0): -1.0, (0, 2): -1.0}
    for L0, L1 in ((ident, ident), (lap, lap)):
        plain = _lib.make_kdesc_array(_lower(lp, kernel, L0, L1))
        assert _lib.lib.lpgp_kron_fits(plain, len(plain)) == 1
        for j in range(2):
            groups = _lower(lp, kernel, L0, L1, dlog=j)
            arr = _lib.make_kdesc_array(groups)
            assert _lib.lib.lpgp_kron_fits(arr, len(arr)) == 0
            Pg = _engine.Points(ctx, X)
            Pg.grid_factors = (_engine.Points(ctx, f0[:, None]), _engine.Points(ctx, f1[:, None]))
            A = _engine.GramMatrix(ctx, 256)
            A.add_block(len(X))
            A.assemble(groups, Pg, None, 0, 0)
            B = _engine.GramMatrix(ctx, 256)
            B.add_block(len(X))
            B.assemble(groups, _engine.Points(ctx, X), None, 0, 0)
            a, b = A.todense(), B.todense()
            assert np.max(np.abs(a - b)) <= ENTRY_RTOL * np.max(np.abs(b))
            ref = ref_block(kernel, L0, L1, X[:40], X[:37], dlog=j)
            assert np.max(np.abs(a[:40, :37] - ref)) <= ENTRY_RTOL * np.max(np.abs(b))
            F0 = (C.c_void_p * 2)(*[f._h for f in Pg.grid_factors])
            assert _lib.lib.lpgp_gram_assemble_grid(ctx._h, arr, len(arr), F0, None, A._h, 0, 0) != 0
            assert b"Kronecker" in _lib.lib.lpgp_last_error()


# ---- the dense inverse ----------------------------------------------------------------------------------------------------------
mat_raw = _hooks.mat_raw


def _refined_inverse(G):
    """(LAPACK's inverse, the inverse refined by Newton steps with long-double residuals)."""
    X0 = np.linalg.inv(G)
    Gl, X = G.astype(np.longdouble), X0.astype(np.longdouble)
    for _ in range(4):
        X = X + X @ (np.eye(len(G), dtype=np.longdouble) - Gl @ X)
    return X0, X


INV_KERNEL = [(1.3, [("matern", 2.5, 0.5)])]


def _value_chain(lp, sizes, seed, noise=1e-2):
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(seed)
    prior = lp.GaussianProcess(lp.functions.Zero((1,)), 1.3 * cf.Matern((1,), nu=2.5, lengthscales=0.5))
    u, blocks = prior, []
    for n in sizes:
        X = rng.uniform(-1, 1, (n, 1))
        Y = np.sin(3 * X[:, 0]) + math.sqrt(noise) * rng.standard_normal(n)
        u = u.condition_on_observations(Y, X, b=lp.randvars.Normal(np.zeros(n), np.full(n, noise)))
        blocks.append(ogp.ObsBlock(X, ocf.identity(1), Y, None, noise))
    return u, ogp.gram(INV_KERNEL, blocks), ogp.residual(blocks)


INVERSE_PANELS = (128, 256, 384, 4096)          # option "inverse_diag_panel": 384 does not divide 640, the last panel is short


def _check_inverse_padding(ctx, ginv, got, sizes):
    """The padded layout of an inverse: every block padded to a multiple of 128 with the identity."""
    raw = mat_raw(ctx, ginv)
    pn, off = raw.shape[0], 0
    assert pn == sum(-(-n // 128) * 128 for n in sizes)
    logical = np.zeros(pn, dtype=bool)
    for n in sizes:
        logical[off:off + n] = True
        off += -(-n // 128) * 128
    low = np.tril(raw)
    pad = np.flatnonzero(~logical)
    assert len(pad) > 0
    assert np.array_equal(low[pad][:, pad], np.eye(len(pad))) and not np.any(low[pad][:, logical]) and not np.any(low[logical][:, pad])
    assert np.array_equal(low[logical][:, logical], np.tril(got))


@pytest.mark.parametrize("sizes", [(200, 317), (129,)], ids=["200+317", "129"])
def test_inverse_against_lapack(lp, ctx, sizes):
    """`inverse()`: the lower triangle against `numpy.linalg.inv` of the oracle's Gram matrix (Matern-5/2, noise 1e-2), relative to
    max |G^-1|, within 4 x LAPACK's own distance from the inverse refined with long-double residuals; the padding rows are the
    identity's; the factor is bitwise unchanged.  At the default column panel (4096: one panel) and at 128, 256 and 384 columns: W = L^-1
    then comes panel by panel, each panel after the first solved against a trailing sub-factor into W + j0 (pn + 1) with leading
    dimension pn (five, three and two panels at 640 padded rows, the last of 384 short; one and two at 256)."""
    from _backward import restored
    u, G, r = _value_chain(lp, sizes, seed=31)
    u._check_current()
    mat = u._state.mat
    before = mat.todense("factor")
    lapack, exact = _refined_inverse(G)
    scale = float(np.max(np.abs(exact)))
    tri = np.tril_indices(len(G))
    e_lap = float(np.max(np.abs(lapack[tri] - exact[tri]))) / scale
    assert np.linalg.cond(G) < 1e6
    assert ctx.get_option("inverse_diag_panel") == 4096
    with restored(ctx, ("inverse_diag_panel",)) as apply:
        for panel in INVERSE_PANELS[::-1]:
            apply({"inverse_diag_panel": panel})
            ginv = mat.inverse()
            assert np.array_equal(mat.todense("factor"), before)
            got = ginv.todense()
            e_dev = float(np.max(np.abs(got[tri] - exact[tri]))) / scale
            print(f"inverse {sizes} panel {panel}: cond2 {np.linalg.cond(G):.2e}  device {e_dev:.2e}, LAPACK {e_lap:.2e} of max |G^-1| from the refined "
                  f"inverse: ratio {e_dev / e_lap:.2f}")
            assert e_dev <= 4.0 * e_lap, (panel, e_dev, e_lap)
            _check_inverse_padding(ctx, ginv, got, sizes)
    assert ctx.get_option("inverse_diag_panel") == 4096


INVERSE_PROBE_RATIO = 1.61       # nine tile rows: probe residual of the device's inverse <= this x LAPACK's (twice the largest measured, 0.804: MEASUREMENTS.md)


def _probe_residual(Gl, norm_G, X, probes):
    """max over the probes v of || v - G (X v) ||_inf / (|| G ||_inf || X ||_inf || v ||_inf), the products in long double."""
    Xl = X.astype(np.longdouble)
    norm_X = float(np.max(np.sum(np.abs(Xl), axis=1)))
    worst = 0.0
    for v in probes:
        vl = v.astype(np.longdouble)
        res = vl - Gl @ (Xl @ vl)
        worst = max(worst, float(np.max(np.abs(res))) / (norm_G * norm_X * float(np.max(np.abs(v)))))
    return worst


def test_inverse_of_nine_tile_rows(lp, ctx):
    """One block of 1100 rows, 1152 padded: nine tile rows, so W^T W runs in bands of 4, 4 and 1 tile columns -- a full-width band at
    a nonzero offset, which the 640 padded rows above (bands of 4 and 1) never have -- at one panel (4096) and at 256 columns (five
    panels, the last of 128).  The refined long-double inverse costs a minute at this size; the measure is the residual on 8 seeded
    probes, max_v || v - G (X v) ||_inf / (|| G ||_inf || X ||_inf || v ||_inf) with the products in long double, against the same
    measure of `numpy.linalg.inv(G)` on the same G and probes: at most INVERSE_PROBE_RATIO x LAPACK's.  Padding and factor as above."""
    from _backward import restored
    sizes = (1100,)
    u, G, r = _value_chain(lp, sizes, seed=32)
    u._check_current()
    mat = u._state.mat
    assert mat.padded_n == 1152
    before = mat.todense("factor")
    assert np.linalg.cond(G) < 1e6
    Gl = G.astype(np.longdouble)
    norm_G = float(np.max(np.sum(np.abs(G), axis=1)))
    probes = np.random.default_rng(1100).standard_normal((8, 1100))
    e_lap = _probe_residual(Gl, norm_G, np.linalg.inv(G), probes)
    with restored(ctx, ("inverse_diag_panel",)) as apply:
        for panel in (256, 4096):
            apply({"inverse_diag_panel": panel})
            ginv = mat.inverse()
            assert np.array_equal(mat.todense("factor"), before)
            got = ginv.todense()
            assert np.array_equal(got, got.T)
            e_dev = _probe_residual(Gl, norm_G, got, probes)
            print(f"inverse (1100,) panel {panel}: probe residual device {e_dev:.3e}, LAPACK {e_lap:.3e}: ratio {e_dev / e_lap:.3f}")
            assert e_dev <= INVERSE_PROBE_RATIO * e_lap, (panel, e_dev, e_lap)
            _check_inverse_padding(ctx, ginv, got, sizes)


def _exact_contraction(ctx, mat, ginv, dG, sizes, caps, diag_caps):
    """Integer operands (tests/_exact_operands.py: integers of [-4, 4] in `ginv`, `dG`, `r` and `v`, NaN and 1e30 in every masked
    position) written over the storage of `ginv` and `dG`; `mat` is the factored identity, so w = r exactly.  Every product and every
    partial sum of evidence_grad_partial_kernel / evidence_grad_final_kernel is then an integer below 2^53: q and t EQUAL the int64
    sums whatever the launch -- `caps`: at most that many workgroups (0: the public call's launch) through `lpgp_test_evidence_grad`,
    `diag_caps` likewise for the diagonal form with v on the last block, scalar = 0."""
    import _exact_operands as ex
    raw, r, v, q_ref, t_ref, diag = ex.contraction_operands(sizes, seed=4000 + sum(sizes))
    n = r.size
    assert ex.contraction_partial_sum_bound(n) < ex.EXACT_LIMIT and mat.n == n
    mat_raw(ctx, ginv, raw["ginv"])
    mat_raw(ctx, dG, raw["dG"])
    rf = r.astype(np.double)
    assert np.array_equal(mat.solve_weights(rf), rf), "a solve against the identity factor does not return r exactly"
    for cap in caps:
        q, t = _hooks.evidence_grad(ctx, mat, ginv, dG, rf, cap)
        print(f"exact contraction {sizes} cap {cap}: q {q!r} (int64 {q_ref}), t {t!r} (int64 {t_ref})")
        assert (q, t) == (float(q_ref), float(t_ref)), (cap, q, t, q_ref, t_ref)
        assert _hooks.evidence_grad(ctx, mat, ginv, dG, rf, cap) == (q, t)
    assert mat.evidence_grad(ginv, dG, rf) == (float(q_ref), float(t_ref))
    bi, lo = len(sizes) - 1, sum(sizes[:-1])
    vb = v[lo:]
    qd_ref, td_ref = int(np.sum(vb * r[lo:] * r[lo:])), int(np.sum(vb * diag[lo:]))
    assert qd_ref != 0 and td_ref != 0
    for cap in diag_caps:
        qd, td = _hooks.evidence_grad_diag(ctx, mat, ginv, bi, rf, v=vb.astype(np.double), scalar=0.0, max_wgs=cap)
        print(f"exact diagonal form {sizes} cap {cap}: q {qd!r} (int64 {qd_ref}), t {td!r} (int64 {td_ref})")
        assert (qd, td) == (float(qd_ref), float(td_ref)), (cap, qd, td, qd_ref, td_ref)
    assert mat.evidence_grad_diag(ginv, bi, rf, v=vb.astype(np.double), scalar=0.0) == (float(qd_ref), float(td_ref))


def test_contraction_second_trip_of_the_final_kernel(ctx):
    """Blocks of 130 + 300 + 700 rows: 1408 padded rows, 352 workgroups of four columns -- more than the 256 threads of
    evidence_grad_final_kernel, whose loop over the partials takes its second trip (pn > 1024; every other case of this file has
    pn <= 640).  Integer operands, exact; a cap of 1 for the other extreme (352 columns per wave)."""
    import _exact_operands as ex
    from linpde_gp_amd import _lib
    sizes = (130, 300, 700)
    mat, ginv, dG = ex.identity_factored(ctx, sizes), ex.cleared(ctx, sizes), ex.cleared(ctx, sizes)
    assert mat.padded_n == 1408 and -(-mat.padded_n // 4) == 352 > 256
    _exact_contraction(ctx, mat, ginv, dG, sizes, caps=(0, 1), diag_caps=(0, 1))
    # the hooks refuse what the public calls refuse
    r = np.ones(mat.n)
    with pytest.raises(_lib.LpgpError, match="must not be factored"):
        _hooks.evidence_grad(ctx, mat, ginv, mat, r, 1)
    with pytest.raises(_lib.LpgpError, match=r"not \(fully\) factored"):
        _hooks.evidence_grad(ctx, dG, ginv, dG, r, 1)
    with pytest.raises(_lib.LpgpError, match="block layout"):
        _hooks.evidence_grad_diag(ctx, mat, ex.cleared(ctx, (1130,)), 2, r, max_wgs=1)
    with pytest.raises(_lib.LpgpError, match="bad block"):
        _hooks.evidence_grad_diag(ctx, mat, ginv, 3, r, max_wgs=1)


def test_contraction_kernel_alone(lp, ctx):
    """`lpgp_mat_evidence_grad` on seeded random lower triangles in the 200 + 317 layout, NaN and 1e30 in every padding row and
    column and above the diagonal: G = I (so w = r exactly), result = `math.fsum` of the logical terms within n eps sum |terms|,
    two calls bit-identical.  A padding leak shows here; so does the diagonal / off-diagonal weight.  Then integer operands under
    the same garbage (`_exact_contraction`): q and t equal the int64 sums for the public launch (one column per wave) and for 1 and 3
    workgroups (160 and 54 columns per wave, the `j += nwaves` loop that otherwise repeats only above 8192 padded rows)."""
    from linpde_gp_amd import _engine
    cf = lp.randprocs.covfuncs
    sizes = (200, 317)
    rng = np.random.default_rng(77)
    zero = (0.0 * cf.ExpQuad((1,), lengthscales=1.0)).lower()
    mats = []
    for _ in range(3):
        M = _engine.GramMatrix(ctx, 640)
        for i, n in enumerate(sizes):
            P = _engine.Points(ctx, rng.uniform(-1, 1, (n, 1)))
            M.add_block(n)
            for j in range(i):
                M.assemble(zero, P, pts[j], i, j)
            M.assemble(zero, P, None, i, i)
            pts = (pts if i else []) + [P]
        mats.append(M)
    mat, ginv, dG = mats
    for i in range(2):
        mat.add_diag(i, scalar=1.0)
    assert mat.potrf() == 0
    pn = mat.padded_n
    assert pn == 256 + 384
    logical = np.zeros(pn, dtype=bool)
    logical[:200] = True
    logical[256:256 + 317] = True
    n = int(logical.sum())
    host = {}
    for name, M in (("ginv", ginv), ("dG", dG)):
        full = rng.standard_normal((pn, pn)) * np.exp(rng.uniform(-3, 3, (pn, pn)))
        garbage = np.where(rng.uniform(size=(pn, pn)) < 0.5, np.nan, 1e30)
        keep = np.tril(np.ones((pn, pn), dtype=bool)) & logical[:, None] & logical[None, :]
        raw = np.where(keep, full, garbage)
        mat_raw(ctx, M, raw)
        host[name] = np.where(keep, full, 0.0)[logical][:, logical]
    r = rng.standard_normal(n)
    A, B = host["ginv"], host["dG"]
    wgt = 2.0 * np.tril(np.ones((n, n)), -1) + np.eye(n)
    tq = (wgt * np.outer(r, r) * B).ravel()
    tt = (wgt * A * B).ravel()
    q_ref, t_ref = math.fsum(tq), math.fsum(tt)
    q, t = mat.evidence_grad(ginv, dG, r)
    print(f"contraction: q {q:.17e} (ref {q_ref:.17e}, bound {n * EPS * np.sum(np.abs(tq)):.2e})  t {t:.17e} (ref {t_ref:.17e}, "
          f"bound {n * EPS * np.sum(np.abs(tt)):.2e})")
    assert math.isfinite(q) and math.isfinite(t)
    # (the products of three factors in q carry two roundings more than a term of fsum's: 3 eps per term, far inside n eps)
    assert abs(q - q_ref) <= n * EPS * np.sum(np.abs(tq))
    assert abs(t - t_ref) <= n * EPS * np.sum(np.abs(tt))
    assert mat.evidence_grad(ginv, dG, r) == (q, t)
    # the diagonal form: dG = diag(v) + s I on block 1
    v = rng.standard_normal(317)
    qd, td = mat.evidence_grad_diag(ginv, 1, r, v=v, scalar=0.25)
    vv = np.concatenate([np.zeros(200), v + 0.25])
    assert abs(qd - math.fsum(vv * r * r)) <= n * EPS * np.sum(np.abs(vv * r * r))
    assert abs(td - math.fsum(vv * np.diag(A))) <= n * EPS * np.sum(np.abs(vv * np.diag(A)))
    # integer operands under the same garbage: exact, for one column per wave (uncapped: 160 workgroups) and for 160 and 54 columns per wave
    _exact_contraction(ctx, mat, ginv, dG, sizes, caps=(0, 1, 3), diag_caps=(0, 1))
    # refusals: another layout, a factored derivative
    from linpde_gp_amd import _lib
    with pytest.raises(_lib.LpgpError, match="block layout"):
        other = _engine.GramMatrix(ctx, 640)
        other.add_block(517)
        mat.evidence_grad(ginv, other, r)
    with pytest.raises(_lib.LpgpError, match="must not be factored"):
        mat.evidence_grad(ginv, mat, r)
    with pytest.raises(_lib.LpgpError, match=r"not \(fully\) factored"):
        dG.inverse()


# ---- the gradient end to end ----------------------------------------------------------------------------------------------------
class Problem:
    """A chain of conditionings described once: the device posterior and the oracle's blocks from the same numbers."""

    def __init__(self, d, kernel, steps):
        self.d, self.kernel, self.steps = d, kernel, steps          # steps: [(X, L dict, Y, noise diagonal or scalar)]

    def posteriors(self, lp, kernel=None, tau=None):
        from linpde_gp_amd.linfuncops import diffops
        kernel = kernel or self.kernel
        k = _device_groups(lp, kernel)
        if self.d == 1:
            k = _as_vector_1d(lp, kernel)
        prior = lp.GaussianProcess(lp.functions.Zero((self.d,)), k)
        u, out = prior, []
        for b, (X, L, Y, noise) in enumerate(self.steps):
            op = None
            if any(sum(mi) for mi in L):
                assert L == {tuple(2 * int(i == j) for i in range(self.d)): -1.0 for j in range(self.d)}
                op = -1.0 * diffops.Laplacian((self.d,))
            nv = np.broadcast_to(np.asarray(noise, dtype=np.double), (len(X),)) * (1.0 if tau is None else tau[b])
            u = u.condition_on_observations(Y, X, L=op, b=lp.randvars.Normal(np.zeros(len(X)), nv.copy()))
            out.append(u)
        return out

    def blocks(self, upto=None):
        return [ogp.ObsBlock(X, L, Y, None, noise) for X, L, Y, noise in self.steps[:upto]]

    def dgram(self, upto=None, group=None, dlog=None):
        """dG / d log(parameter) as float64: one summand alone (its output scale) or its lengthscale derivative, from the 50-digit entries."""
        st = self.steps[:upto]
        if len(self.kernel) == 1 and dlog is None:       # the only summand by its output scale: the Gram matrix without its noise
            return ogp.gram(self.kernel, [ogp.ObsBlock(X, L, Y, None, None) for X, L, Y, _ in st])
        rows = []
        for i, (Xi, Li, _, _) in enumerate(st):
            rows.append([ref_block(self.kernel, Li, Lj, Xi, Xj, group=group, dlog=dlog) for (Xj, Lj, _, _) in st[:i + 1]])
        n = [len(s[0]) for s in st]
        off = np.cumsum([0] + n)
        out = np.zeros((off[-1], off[-1]))
        for i in range(len(st)):
            for j in range(i + 1):
                out[off[i]:off[i + 1], off[j]:off[j + 1]] = rows[i][j]
                out[off[j]:off[j + 1], off[i]:off[i + 1]] = rows[i][j].T
        return out

    def dnoise(self, b, upto=None):
        st = self.steps[:upto]
        n = [len(s[0]) for s in st]
        off = np.cumsum([0] + n)
        out = np.zeros((off[-1], off[-1]))
        idx = np.arange(off[b], off[b + 1])
        out[idx, idx] = np.broadcast_to(np.asarray(st[b][3], dtype=np.double), (n[b],))
        return out


def _as_vector_1d(lp, kernel):
    cf = lp.randprocs.covfuncs
    summands = [s * (cf.Matern((1,), nu=f[0][1], lengthscales=f[0][2]) if f[0][0] == "matern" else cf.ExpQuad((1,), lengthscales=f[0][1]))
                for s, f in kernel]
    k = summands[0]
    for s in summands[1:]:
        k = k + s
    return k


def _problem(name):
    rng = np.random.default_rng({"a": 5, "b": 6, "c": 7}[name])
    if name == "a":        # 1-D Matern-5/2, 2^2, l = 0.3: 70 noisy values, then 130 values of -Laplacian with diagonal noise
        kernel = [(4.0, [("matern", 2.5, 0.3)])]
        X0 = rng.uniform(-1, 1, (70, 1))
        Y0 = np.sin(3 * X0[:, 0]) + 0.1 * rng.standard_normal(70)
        X1 = rng.uniform(-1, 1, (130, 1))
        nz = rng.uniform(0.5, 1.5, 130)
        Y1 = 9 * np.sin(3 * X1[:, 0]) + np.sqrt(nz) * rng.standard_normal(130)
        return Problem(1, kernel, [(X0, {(0,): 1.0}, Y0, 1e-2), (X1, {(2,): -1.0}, Y1, nz)])
    if name == "b":        # 2-D Matern-5/2 x ExpQuad, two lengthscales: 150 scattered values, noise 1e-2
        kernel = [(1.5, [("matern", 2.5, 0.6), ("expquad", 0.35)])]
        X = rng.uniform(-1, 1, (150, 2))
        Y = np.sin(2 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.1 * rng.standard_normal(150)
        return Problem(2, kernel, [(X, {(0, 0): 1.0}, Y, 1e-2)])
    kernel = [(1.5, [("matern", 2.5, 0.4)]), (0.7, [("expquad", 0.9)])]      # c: a sum of two scaled kernels on 96 points
    X = rng.uniform(-1, 1, (96, 1))
    Y = np.sin(3 * X[:, 0]) + 0.3 * X[:, 0] + 0.1 * rng.standard_normal(96)
    return Problem(1, kernel, [(X, {(0,): 1.0}, Y, 1e-2)])


def _parameters(prob, upto=None):
    nb = len(prob.steps[:upto])
    out = [("log_output_scale", (g,), dict(group=g)) for g in range(len(prob.kernel))]
    out += [("log_lengthscales", (g, j), dict(group=g, dlog=j)) for g in range(len(prob.kernel)) for j in range(prob.d)]
    out += [("log_noise", (b,), dict(noise=b)) for b in range(nb)]
    return out


def _dmatrix(prob, spec, upto=None):
    return prob.dnoise(spec["noise"], upto) if "noise" in spec else prob.dgram(upto, **spec)


def _grad_lapack(G, r, dGs):
    w = scipy.linalg.cho_solve(scipy.linalg.cho_factor(G, lower=True), r)
    Gi = np.linalg.inv(G)
    return np.array([0.5 * (w @ dG @ w) - 0.5 * np.sum(Gi * dG) for dG in dGs])


def _grad_refined(G, r, dGs):
    """The same in long double with the solve and the inverse refined by long-double residuals."""
    _, Gi = _refined_inverse(G)
    Gl, rl = G.astype(np.longdouble), r.astype(np.longdouble)
    w = Gi @ rl
    for _ in range(4):
        w = w + Gi @ (rl - Gl @ w)
    return np.array([np.longdouble(0.5) * (w @ dG.astype(np.longdouble) @ w) - np.longdouble(0.5) * np.sum(Gi * dG.astype(np.longdouble)) for dG in dGs])


def _grad_mpmath(prob):
    """Case (c) entirely in 50-digit arithmetic: G and every dG from the 50-digit entries, Cholesky, W = L^-1, G^-1 = W^T W."""
    with mpmath.workdps(DPS):
        (X, L, Y, noise), = prob.steps
        n = len(X)
        G = ref_block_mp(prob.kernel, L, L, X, X)
        for i in range(n):
            G[i, i] += mpmath.mpf(float(noise))
        r = np.array([mpmath.mpf(float(y)) for y in Y], dtype=object)
        Lc = np.zeros((n, n), dtype=object)
        for j in range(n):
            Lc[j, j] = mpmath.sqrt(G[j, j] - (Lc[j, :j] @ Lc[j, :j] if j else 0))
            if j + 1 < n:
                Lc[j + 1:, j] = (G[j + 1:, j] - (Lc[j + 1:, :j] @ Lc[j, :j] if j else 0)) / Lc[j, j]
        W = np.zeros((n, n), dtype=object)
        for i in range(n):                            # rows of L^-1 by forward substitution
            e = np.zeros(n, dtype=object)
            e[i] = mpmath.mpf(1)
            W[i, :i + 1] = (e[:i + 1] - (Lc[i, :i] @ W[:i, :i + 1] if i else 0)) / Lc[i, i]
        Gi = W.T @ W
        w = Gi @ r
        out = []
        for _, _, spec in _parameters(prob):
            if "noise" in spec:
                dG = np.zeros((n, n), dtype=object)
                for i in range(n):
                    dG[i, i] = mpmath.mpf(float(noise))
            else:
                dG = ref_block_mp(prob.kernel, L, L, X, X, **spec)
            out.append((w @ dG @ w) / 2 - np.sum(Gi * dG) / 2)
        return np.array([float(v) for v in out], dtype=np.longdouble)


def _flat(g, prob, upto=None):
    return np.array([getattr(g, field)[idx] for field, idx, _ in _parameters(prob, upto)])


_measured = {}


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_gradient_against_gpml_5_9(lp, name):
    """Every component of `log_marginal_likelihood_gradient()` against GPML eq. 5.9 on the oracle's Gram matrix with dG from the
    50-digit entries: within 4 x LAPACK's own distance from the long-double-refined evaluation (case c: from the evaluation entirely
    in 50-digit arithmetic), or 1e-12 relative.  `value` is `log_marginal_likelihood()` exactly; the first posterior of chain (a)
    answers for its 70 rows, before and after the second conditioning is looked at.  Sanity: a central difference of
    `log_marginal_likelihood()` over re-conditioned priors, step 1e-4 in the log parameter, 1e-5 relative."""
    prob = _problem(name)
    posts = prob.posteriors(lp)
    views = [(len(posts), posts[-1])] + ([(1, posts[0])] if name == "a" else [])
    for upto, u in views:
        blocks = prob.blocks(upto)
        G, r = ogp.gram(prob.kernel, blocks), ogp.residual(blocks)
        params = _parameters(prob, upto)
        dGs = [_dmatrix(prob, spec, upto) for _, _, spec in params]
        lapack = _grad_lapack(G, r, dGs)
        exact = _grad_mpmath(prob) if name == "c" else _grad_refined(G, r, dGs)
        g = u.log_marginal_likelihood_gradient()
        assert g.value == u.log_marginal_likelihood()
        assert g.log_output_scale.shape == (len(prob.kernel),) and g.log_lengthscales.shape == (len(prob.kernel), prob.d)
        assert g.log_noise.shape == (upto,)
        dev = _flat(g, prob, upto)
        for (field, idx, _), d_, l_, e_ in zip(params, dev, lapack, exact):
            e_dev, e_lap = abs(float(d_ - e_)), abs(float(l_ - e_))
            print(f"case {name} [{upto} block(s)] {field}{list(idx)}: exact {float(e_):+.15e}  device off by {e_dev:.2e} ({e_dev / abs(float(e_)):.1e} rel), "
                  f"LAPACK by {e_lap:.2e} ({e_lap / abs(float(e_)):.1e} rel)   cond2 {np.linalg.cond(G):.1e}")
            assert e_dev <= max(4.0 * e_lap, 1e-12 * abs(float(e_))), (name, upto, field, idx, e_dev, e_lap)
        _measured[(name, upto)] = dev
        if upto < len(posts):
            again = _flat(posts[0].log_marginal_likelihood_gradient(), prob, upto)       # (the view went to the longer chain and back)
            assert np.array_equal(again, dev)
            assert np.array_equal(_flat(posts[-1].log_marginal_likelihood_gradient(), prob), _measured[(name, len(posts))])
    # sanity, not the criterion: central differences of the evidence over re-conditioned priors
    h = 1e-4
    full = _measured[(name, len(posts))]
    for (field, idx, spec), want in zip(_parameters(prob), full):
        vals = []
        for s in (+h, -h):
            kernel = [(sc, list(fs)) for sc, fs in prob.kernel]
            tau = [1.0] * len(prob.steps)
            if "noise" in spec:
                tau[spec["noise"]] = math.exp(s)
            elif "dlog" in spec:
                f = list(kernel[spec["group"]][1][spec["dlog"]])
                f[-1] = f[-1] * math.exp(s)
                kernel[spec["group"]][1][spec["dlog"]] = tuple(f)
            else:
                kernel[spec["group"]] = (kernel[spec["group"]][0] * math.exp(s), kernel[spec["group"]][1])
            vals.append(prob.posteriors(lp, kernel, tau)[-1].log_marginal_likelihood())
        fd = (vals[0] - vals[1]) / (2 * h)
        print(f"case {name} {field}{list(idx)}: central difference {fd:+.10e}, analytic {want:+.10e}")
        assert abs(fd - want) <= 1e-5 * max(abs(want), abs(fd)), (name, field, idx, fd, want)


def test_modes_and_refusals(lp):
    from linpde_gp_amd import _engine, _spawn
    cf = lp.randprocs.covfuncs
    prob = _problem("a")
    eager = _flat(prob.posteriors(lp)[-1].log_marginal_likelihood_gradient(), prob)
    saved = lp.config.lazy_factorization
    lp.config.lazy_factorization = True
    try:
        lazy = _flat(prob.posteriors(lp)[-1].log_marginal_likelihood_gradient(), prob)
        assert np.all(np.abs(lazy - eager) <= 1e-12 * np.abs(eager))
        # a block that is not positive definite is dropped at the first use: LinAlgError, again on every later use
        prior = lp.GaussianProcess(lp.functions.Zero((1,)), cf.ExpQuad((1,), lengthscales=1.0))
        X = np.array([[0.0], [0.0], [0.5]])
        bad = prior.condition_on_observations(np.zeros(3), X, b=lp.randvars.Normal(np.zeros(3), -1e-3 * np.eye(3)))
        for _ in range(2):
            with pytest.raises(np.linalg.LinAlgError):
                bad.log_marginal_likelihood_gradient()
    finally:
        lp.config.lazy_factorization = saved
    prior = lp.GaussianProcess(lp.functions.Zero((1,)), cf.ExpQuad((1,), lengthscales=1.0))
    # nothing observed: zeros of the right shapes
    empty = prior.condition_on_observations(np.zeros(0), np.zeros((0, 1))).log_marginal_likelihood_gradient()
    assert empty.value == 0.0 and empty.log_output_scale.tolist() == [0.0] and empty.log_lengthscales.tolist() == [[0.0]] and empty.log_noise.shape == (0,)
    # a block without noise: its entry is 0.0
    Xn = np.linspace(-1, 1, 9)[:, None]
    k52 = lp.GaussianProcess(lp.functions.Zero((1,)), cf.Matern((1,), nu=2.5, lengthscales=0.2))
    assert k52.condition_on_observations(np.sin(Xn[:, 0]), Xn).log_marginal_likelihood_gradient().log_noise.tolist() == [0.0]
    # a dense noise covariance goes through the scratch matrix: the same number as the diagonal form where they coincide
    rng = np.random.default_rng(3)
    Xd, Yd = rng.uniform(-1, 1, (40, 1)), rng.standard_normal(40)
    A = rng.standard_normal((40, 40))
    dense = 1e-2 * np.eye(40) + 1e-3 * (A @ A.T) / 40
    gd = k52.condition_on_observations(Yd, Xd, b=lp.randvars.Normal(np.zeros(40), dense)).log_marginal_likelihood_gradient()
    Gd = ocf.LkL([(1.0, [("matern", 2.5, 0.2)])], {(0,): 1.0}, {(0,): 1.0}, Xd, Xd) + dense
    wd = np.linalg.solve(Gd, Yd)
    want = 0.5 * wd @ dense @ wd - 0.5 * np.sum(np.linalg.inv(Gd) * dense)
    assert abs(gd.log_noise[0] - want) <= 1e-9 * abs(want)
    # a matrix-free posterior
    X, Y = np.linspace(-1, 1, 20)[:, None], np.zeros(20)
    saved = lp.config.matrix_free
    lp.config.matrix_free = True
    try:
        mf = prior.condition_on_observations(Y, X, b=lp.randvars.Normal(np.zeros(20), 1e-2 * np.eye(20)))
    finally:
        lp.config.matrix_free = saved
    with pytest.raises(NotImplementedError):
        mf.log_marginal_likelihood_gradient()
    # an isotropic multivariate Matern prior: the whole call
    iso = lp.GaussianProcess(lp.functions.Zero((2,)), cf.Matern((2,), nu=2.5, lengthscales=[0.5, 0.8]))
    X2 = np.random.default_rng(1).uniform(-1, 1, (30, 2))
    ui = iso.condition_on_observations(np.zeros(30), X2, b=lp.randvars.Normal(np.zeros(30), 1e-2 * np.eye(30)))
    with pytest.raises(NotImplementedError, match="isotropic"):
        ui.log_marginal_likelihood_gradient()
    # spawn proxy (no worker group is started) and a context inside a multi-GPU job: refused at the Python level
    proxy = _spawn.RemoteConditionalGaussianProcess.__new__(_spawn.RemoteConditionalGaussianProcess)
    with pytest.raises(NotImplementedError, match="lp.spawn"):
        proxy.log_marginal_likelihood_gradient()
    u = prob.posteriors(lp)[-1]
    dctx = _engine.default_context()
    dctx.distributed = True
    try:
        with pytest.raises(NotImplementedError, match="multi-GPU"):
            u.log_marginal_likelihood_gradient()
    finally:
        dctx.distributed = False
