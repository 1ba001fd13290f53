"""Entry-exact tests of the per-entry evaluation core on SCATTERED points: the assembly kernels `assemble_kernel<D, FACTORS, VAR>` and
`assemble_fast_kernel<D, N0, N1, MODE>`, and the matrix-free product `matvec_kernel` / `matvec_fast_kernel` + `mv_reduce_kernel`.

Assembly.  Every entry a call is supposed to write -- the whole block of `_engine.kernel_matrix`, an off-diagonal block and the lower
triangle of a diagonal block of a `GramMatrix` behind a 37-row scattered block -- is compared with the high-precision reference of
tests/_entry_reference.py:  |got - G| <= K W + eta,  W the envelope weighted by (1 + rho), eta the gradual-underflow term, K measured
on the CPU (tests/test_entry_reference.py, which also shows that the host instantiation of the same code meets the bound on these
very inputs and that a wrong sign, an exchanged dimension or a shifted column misses it by > 1e6 K).  Nothing is scaled by a norm and
no entry is left out; beyond the clamp of the exponential the entry must be exactly +-0; everything outside the block must read
back bit-identical.  The case id names the instantiation the host picks (`_entry_reference.kernel_name`, a restatement of
`fast_shape` / `fast_mode` / `asm_flags` of csrc/assemble.hip).

Product.  y = K(X0, X1) V against sum_j G_ij v_j in long double, row by row:  sum_j B_ij |v_j| + depth u sum_j E_ij |v_j|, B the
entry bound and depth the longest chain of additions, restated from the kernels (`_entry_reference.product_depth`).  The large cases
take their row count from the device's CU count so that a split owns SEVERAL column tiles (per = 2) and, in one of them, the last
split owns none -- what every matrix-free solve beyond ~32k points runs; the plan is asserted before anything is compared."""
import numpy as np
import pytest

import _entry_reference as er
from _backward import restored
from test_gpu_kron_exact import _covfunc, _operator

pytestmark = pytest.mark.gpu

EPS, LD = er.EPS, er.LD
CASES = er.CASES
SCATTERED = 37
ASSEMBLY = [(c, f) for c in CASES for f in ((0, 1) if c.factored else (0,))]


@pytest.fixture(scope="module")
def lp():
    import linpde_gp_amd
    return linpde_gp_amd


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


def _lowered(lp, kernel, L0, L1):
    A, B = _operator(L0), _operator(L1)
    assert {tuple(m): c for m, c in A.coefficients_dict().items()} == L0        # the reference's c_t are the operators' own
    assert {tuple(m): c for m, c in B.coefficients_dict().items()} == L1
    return A(B(_covfunc(lp, kernel), argnum=1), argnum=0).lower()


def _hold(what, got, B, K, mask=None):
    """Every (masked) entry within K W + eta, exactly +-0 beyond the clamp; returns the worst ratio in eps."""
    n1 = got.shape[1]
    mask = np.ones(got.shape, dtype=bool) if mask is None else mask
    ratio, pos = B.ratio(got, mask)
    print(f"device {what}: {ratio / EPS:.2f} eps at {divmod(pos, n1)} (rho = {float(B.rho.reshape(-1)[pos]):.3g}, K = {K / EPS:.2f} eps)")
    err = np.abs(got.astype(LD) - B.G)
    bad = mask & ~(err <= B.bound(K))
    if bad.any():
        i, j = divmod(int(np.flatnonzero(bad)[0]), n1)
        pytest.fail(f"{what}: {int(bad.sum())} of {int(mask.sum())} entries beyond K W + eta; first at ({i}, {j}): got {got[i, j]!r}, "
                    f"reference {float(B.G[i, j])!r}, W {float(B.W[i, j])!r}, eta {float(B.eta[i, j])!r}, rho {float(B.rho[i, j]):.4g}; "
                    f"worst ratio {ratio / EPS:.2f} eps at {divmod(pos, n1)}")
    zero = mask & (B.expo > er.EXP_CLAMP + 1)
    assert np.all(got[zero] == 0.0), f"{what}: an entry beyond the clamp of the exponential is not +-0"
    return ratio / EPS


def _gram_block(ctx, lp, kd, k_plain, D, X0, X1, kind):
    """The block of a GramMatrix behind a 37-row scattered block, and the matrix before / after its assembly."""
    from linpde_gp_amd import _engine
    n0, n1 = X0.shape[0], X1.shape[0]
    Xs = np.random.default_rng(D).uniform(0.0, 3.0, (SCATTERED, D))
    mat = _engine.GramMatrix(ctx, SCATTERED + n0 + (n1 if kind == "off" else 0))
    mat.add_block(SCATTERED)
    mat.assemble(k_plain, _engine.Points(ctx, Xs), None, 0, 0)
    Pr = _engine.Points(ctx, np.ascontiguousarray(X0))
    if kind == "off":
        Pc = _engine.Points(ctx, np.ascontiguousarray(X1))
        bj, bi = mat.add_block(n1), mat.add_block(n0)
        r0, c0 = SCATTERED + n1, SCATTERED
    else:
        Pc = None
        bi = bj = mat.add_block(n0)
        r0 = c0 = SCATTERED
    before = mat.todense("gram")
    mat.assemble(kd, Pr, Pc, bi, bj)
    after = mat.todense("gram")
    # nothing outside the block was written (the lower triangle is what `todense` reads; it mirrors it)
    outside = np.tril(np.ones(after.shape, dtype=bool))
    outside[r0:r0 + n0, c0:c0 + n1] = False
    assert np.array_equal(before.view(np.uint64)[outside], after.view(np.uint64)[outside]), "a write outside the block"
    return after[r0:r0 + n0, c0:c0 + n1]


@pytest.mark.parametrize("case,factors", ASSEMBLY, ids=[er.kernel_name(c.kernel, c.L0, c.L1, bool(f)) + c.id[len(c.expected):] for c, f in ASSEMBLY])
def test_assembly_entry_by_entry(lp, ctx, case, factors):
    from linpde_gp_amd import _engine
    assert er.kernel_name(case.kernel, case.L0, case.L1) == case.expected
    kd = _lowered(lp, case.kernel, case.L0, case.L1)
    X0, X1 = case.points()
    B = case.reference()
    if factors and case.pset == "c":
        ok, bad = er.factor_tiles(case.kernel, X0, X1, lower=case.kind == "diag")
        assert ok >= 1 and bad >= 1, "tiles that keep their per-point factors and tiles that fall back must both occur"
    with restored(ctx, ["asm_factors"]) as apply:
        apply({"asm_factors": factors})
        if case.kind == "off":
            got = _engine.kernel_matrix(ctx, kd, _engine.Points(ctx, np.ascontiguousarray(X0)), _engine.Points(ctx, np.ascontiguousarray(X1)))
            _hold(f"{case.id} factors={factors} kernel_matrix", got, B, er.K_ENTRY)
        got = _gram_block(ctx, lp, kd, _covfunc(lp, case.kernel).lower(), case.D, X0, X1, case.kind)
    _hold(f"{case.id} factors={factors} gram", got, B, er.K_ENTRY, case.mask())


ISO = er.iso_first_cases()


@pytest.mark.parametrize("cid", [c[0] for c in ISO])
def test_iso_first_order_entry_by_entry(lp, ctx, cid):
    """The first-order isotropic group (`DevGroup::iso == 1`: value, directional derivative, the mixed u^T B u term) of the generic
    kernel against the 50-digit blocks of tests/golden/iso_first.npz."""
    from linpde_gp_amd import _engine, _lib
    _, d, p, ls, L0, L1, X0, X1, B = next(c for c in ISO if c[0] == cid)
    k = lp.randprocs.covfuncs.Matern((d,), nu=p + 0.5, lengthscales=ls)
    kd = _operator(L0)(_operator(L1)(k, argnum=1), argnum=0).lower()
    assert len(kd) == 1 and kd[0]["family"] == [_lib.MATERN_ISO] * d
    got = _engine.kernel_matrix(ctx, kd, _engine.Points(ctx, np.ascontiguousarray(X0)), _engine.Points(ctx, np.ascontiguousarray(X1)))
    _hold(f"assemble<{d},->-iso-{cid} kernel_matrix", got, B, er.K_ISO_FIRST)
    got = _gram_block(ctx, lp, kd, k.lower(), d, X0, X1, "off")
    _hold(f"assemble<{d},->-iso-{cid} gram", got, B, er.K_ISO_FIRST)


# ---- the matrix-free product -------------------------------------------------------------------------------------------------------
def _hold_rows(what, got, y, bound):
    err = np.abs(got.astype(LD) - y)
    ratio = float(np.max(err / bound))
    print(f"device product {what}: worst |err| / bound = {ratio:.3f}")
    assert np.all(err <= bound), f"{what}: a row beyond its bound ({ratio:.3f} of it); first at {np.argwhere(~(err <= bound))[0]}"
    return ratio


_small = {}


@pytest.mark.parametrize("name,desc,factors", er.PRODUCT_SMALL, ids=[p[0] for p in er.PRODUCT_SMALL])
def test_small_product_row_by_row(lp, ctx, name, desc, factors):
    """(130, 150) with 1, 4, 5 and 9 right-hand sides (one pass of MV_RHS and a second, ragged one), through `linop @ V`,
    `kernel_matvec` and `kernel_matvec_dev` (accumulate 0 and 1, row offsets that are no multiple of 64)."""
    from linpde_gp_amd import _engine
    if desc not in _small:
        _small[desc] = er.small_product_block(desc)
    X0, X1, B = _small[desc]
    n0, n1 = er.PRODUCT_SHAPE
    if desc == "iso":
        q = er.ISO_PRODUCT
        L0, L1 = er.iso_first_pairs(3, q["v"], q["w"], q["c"])["grad_grad"]
        kk = _operator(L0)(_operator(L1)(q["scale"] * lp.randprocs.covfuncs.Matern((3,), nu=q["p"] + 0.5, lengthscales=np.array(q["lengthscales"])),
                                         argnum=1), argnum=0)
        K = er.K_ISO_FIRST
    else:
        kernel, L0, L1 = er.DESCRIPTORS[desc]
        kk = _operator(L0)(_operator(L1)(_covfunc(lp, kernel), argnum=1), argnum=0)
        assert name.startswith(er.kernel_name(kernel, L0, L1, bool(factors), product=True))
        K = er.K_ENTRY
    kd = kk.lower()
    tiles_r, tiles_c, splits, per, owned = er.split_plan(n0, n1, ctx.device_info()["cus"])
    assert (tiles_r, tiles_c, splits, per) == (3, 3, 3, 1)
    P0, P1 = _engine.Points(ctx, np.ascontiguousarray(X0)), _engine.Points(ctx, np.ascontiguousarray(X1))
    v_off, y_off = 3, 5
    with restored(ctx, ["asm_factors"]) as apply:
        apply({"asm_factors": factors})
        for m in er.PRODUCT_RHS:
            V = np.random.default_rng(m).standard_normal((n1, m))
            y, bound = er.product_reference(B, V, K, per, splits)
            _hold_rows(f"{name} m={m} kernel_matvec", _engine.kernel_matvec(ctx, kd, P0, P1, V), y, bound)
            if not factors:
                got = kk.linop(X0, X1) @ V
                _hold_rows(f"{name} m={m} linop", np.asarray(got).reshape(n0, m), y, bound)
            rng = np.random.default_rng(100 + m)
            Vh, old = rng.standard_normal((n1 + 7, m)), rng.standard_normal((n0 + 9, m))
            Vh[v_off:v_off + n1] = V
            Vd = _engine.DeviceVectors(ctx, n1 + 7, m, Vh)
            keep = np.ones(n0 + 9, dtype=bool)
            keep[y_off:y_off + n0] = False
            for accumulate in (False, True):
                Y = _engine.DeviceVectors(ctx, n0 + 9, m, old)
                _engine.kernel_matvec_dev(ctx, kd, P0, P1, Vd, v_off, Y, y_off, accumulate)
                got = Y.get()
                assert np.array_equal(got[keep].view(np.uint64), old[keep].view(np.uint64)), f"{name}: a row outside the target moved"
                ya, ba = er.product_reference(B, V, K, per, splits, accumulate, old[y_off:y_off + n0])
                _hold_rows(f"{name} m={m} kernel_matvec_dev accumulate={int(accumulate)}", got[y_off:y_off + n0], ya, ba)


@pytest.mark.parametrize("desc", er.PRODUCT_BIG_DESCRIPTORS)
@pytest.mark.parametrize("name", [c[0] for c in er.PRODUCT_BIG])
def test_product_over_several_tiles_per_split(lp, ctx, name, desc):
    """The accumulation over the column tiles of one split (per = 2) and the split that owns no tile: row counts taken from the CU
    count, the plan asserted from the restated host formula, about 96 sampled rows against the reference, every other row finite,
    and through `kernel_matvec_dev` the rows outside the target keep their bits."""
    from linpde_gp_amd import _engine
    cus = ctx.device_info()["cus"]
    _, n0_of, n1, (splits_w, per_w, owned_w) = next(c for c in er.PRODUCT_BIG if c[0] == name)
    n0 = n0_of(cus)
    tiles_r, tiles_c, splits, per, owned = er.split_plan(n0, n1, cus)
    assert (splits, per, owned) == (splits_w, per_w, owned_w), f"{cus} CUs: tiles {tiles_r} x {tiles_c} give splits {splits}, per {per}, tiles per split {owned}"
    kernel, L0, L1 = er.DESCRIPTORS[desc]
    kd = _lowered(lp, kernel, L0, L1)
    X0, X1, V, rows, B = er.big_product(name, desc, cus)
    m = V.shape[1]
    P0, P1 = _engine.Points(ctx, X0), _engine.Points(ctx, X1)
    y, bound = er.product_reference(B, V, er.K_ENTRY, per, splits)
    got = _engine.kernel_matvec(ctx, kd, P0, P1, V)
    assert got.shape == (n0, m) and np.all(np.isfinite(got))
    what = f"{er.kernel_name(kernel, L0, L1, product=True)}-{name}"
    _hold_rows(f"{what} kernel_matvec", got[rows], y, bound)
    v_off, y_off = 3, 5
    rng = np.random.default_rng(n0)
    Vh, old = rng.standard_normal((n1 + 7, m)), rng.standard_normal((n0 + 9, m))
    Vh[v_off:v_off + n1] = V
    Vd = _engine.DeviceVectors(ctx, n1 + 7, m, Vh)
    keep = np.ones(n0 + 9, dtype=bool)
    keep[y_off:y_off + n0] = False
    for accumulate in (False, True):
        Y = _engine.DeviceVectors(ctx, n0 + 9, m, old)
        _engine.kernel_matvec_dev(ctx, kd, P0, P1, Vd, v_off, Y, y_off, accumulate)
        out = Y.get()
        assert np.array_equal(out[keep].view(np.uint64), old[keep].view(np.uint64)), f"{what}: a row outside the target moved"
        assert np.all(np.isfinite(out))
        ya, ba = er.product_reference(B, V, er.K_ENTRY, per, splits, accumulate, old[y_off:y_off + n0][rows])
        _hold_rows(f"{what} kernel_matvec_dev accumulate={int(accumulate)}", out[y_off:y_off + n0][rows], ya, ba)
