"""Entry-exact tests of the tensor-grid (Kronecker) Gram assembly `lpgp_gram_assemble_grid` -> `launch_assemble_kron`.

Every case builds a `GramMatrix` by hand (a scattered block of 37 rows first, so the grid blocks sit at non-zero row and column
offsets behind a block that is no multiple of the 128-row tile), assembles ONE grid block and compares EVERY entry that call is
supposed to write -- the whole off-diagonal block, the lower triangle of a diagonal block -- with the high-precision reference of
tests/_kron_reference.py:  |got - G| <= K * E  entry by entry, E the envelope (the closed form with absolute coefficients).  No
entry is left out and nothing is scaled by a norm.  Everything outside the block must read back bit-identical to before.

The inputs make a wrong index visible: the factor coordinates are sorted RANDOM points (no factor matrix is Toeplitz, so a shifted
index changes the numbers), a seed of its own per dimension and side, row and column grids differ in every extent, every dimension
has its own kernel family / smoothness / lengthscale, and every case has an operator of odd order in the fastest dimension, whose
factor is antisymmetric: a transposed, shifted or swapped factor is off by O(E).  tests/test_kron_reference.py proves on the CPU
that a transposed factor misses the bound by more than 1e6 K on every case.

The case id names the kernel the dispatcher picks for the shape (`_kron_reference.selected_kernel`, which restates the `if` of
`launch_assemble_kron`); the `assemble_grid` profiling slot proves that the Kronecker path ran.  The same cases run once more
through the per-entry kernels (`config.use_grid_assembly = False`; generic and specialised, D = 2 ... 4) against the same reference
and bound.  Not covered: the multi-GPU instantiation `kron2_kernel<*, true>`."""
import numpy as np
import pytest

import _kron_reference as kr
from _backward import restored

pytestmark = pytest.mark.gpu

# The bound: K = 4 * max over the cases of rho_oracle, rho_oracle = max |oracle.covfuncs.LkL - G| / E the distance of a plain
# NumPy float64 evaluation of the same closed form from the reference (tests/test_kron_reference.py prints it per case; the table
# is in MEASUREMENTS.md, "Entry-exact Kronecker assembly").  The factor 4: the device multiplies D rounded factors and sums T terms
# where the oracle evaluates directly, and uses another exponential.  A wrong index is off by ~E, eleven orders above.
# Measured: max rho_oracle = 6.66 eps (eps = 2^-53; case kron_expand<3,2>-off-t), so K = 26.64 eps = 2.96e-15, above the floor 8 eps.
RHO_ORACLE_MAX = 6.66 * kr.EPS
K = max(4 * RHO_ORACLE_MAX, 8 * kr.EPS)

CASES = kr.CASES
SCATTERED = 37


def _covfunc(lp, kernel):
    cf = lp.randprocs.covfuncs
    k = None
    for scale, factors in kernel:
        kg = scale * cf.TensorProduct(*(cf.Matern((), nu=f[1], lengthscales=f[2]) if f[0] == "matern"
                                        else cf.ExpQuad((), lengthscales=f[1]) for f in factors))
        k = kg if k is None else k + kg
    return k


def _operator(coef):
    from linpde_gp_amd.linfuncops import diffops
    from linpde_gp_amd.linfuncops.diffops._coefficients import MultiIndex, PartialDerivativeCoefficients
    d = len(next(iter(coef)))
    pdc = PartialDerivativeCoefficients({(): {MultiIndex(a): c for a, c in coef.items()}}, (d,), ())
    return diffops.LinearDifferentialOperator(pdc, ((d,), ()))


@pytest.fixture(scope="module")
def lp():
    import linpde_gp_amd
    return linpde_gp_amd


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


@pytest.mark.parametrize("path", ["kron", "entry"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_grid_block_entry_by_entry(lp, ctx, kronecker_everywhere, case, path):
    from linpde_gp_amd import _engine, _lib, config, domains
    k = _covfunc(lp, case.kernel)
    A, B = _operator(case.L0), _operator(case.L1)
    assert {tuple(m): c for m, c in A.coefficients_dict().items()} == case.L0        # the reference's c_t are the operators' own
    assert {tuple(m): c for m, c in B.coefficients_dict().items()} == case.L1
    kd = A(B(k, argnum=1), argnum=0).lower()
    arr = _lib.make_kdesc_array(kd)
    assert _lib.lib.lpgp_kron_fits(arr, len(arr))
    G, E = case.reference()
    n0, n1 = case.shape
    D = case.D
    saved = config.use_grid_assembly
    config.use_grid_assembly = path == "kron"
    try:
        with restored(ctx, ["kron_wide"]) as apply:
            apply({"kron_wide": int(case.kron_wide)})
            Xs = np.random.default_rng(D).uniform(0.0, 1.5, (SCATTERED, D))
            Xr = domains.TensorProductGrid(*case.F0)
            Pr = _engine.as_points(ctx, Xr, np.asarray(Xr).reshape(-1, D))
            assert (Pr.grid_factors is not None) == (path == "kron")
            mat = _engine.GramMatrix(ctx, SCATTERED + n0 + (n1 if case.kind == "off" else 0))
            mat.add_block(SCATTERED)
            mat.assemble(k.lower(), _engine.Points(ctx, Xs), None, 0, 0)
            if case.kind == "off":
                Xc = domains.TensorProductGrid(*case.F1)
                Pc = _engine.as_points(ctx, Xc, np.asarray(Xc).reshape(-1, D))
                bj, bi = mat.add_block(n1), mat.add_block(n0)
                r0, c0 = SCATTERED + n1, SCATTERED
            else:
                Pc = None
                bi = bj = mat.add_block(n0)
                r0 = c0 = SCATTERED
            before = mat.todense("gram")
            ctx.profile_reset()
            ctx.profile_enable(["assemble_grid"])
            mat.assemble(kd, Pr, Pc, bi, bj)
            after = mat.todense("gram")
            launches = ctx.profile_get()["assemble_grid"]["launches"]
            ctx.profile_enable(False)
    finally:
        config.use_grid_assembly = saved
    assert launches >= 1 if path == "kron" else launches == 0, f"{case.id}: {launches} launches of the Kronecker expansion"
    got = after[r0:r0 + n0, c0:c0 + n1]
    mask = case.mask()
    ratio, pos = kr.worst_ratio(got, G, E, mask)
    print(f"device {path} {case.id}: {ratio / kr.EPS:.2f} eps at {case.describe(pos)}")
    err = np.abs(got.astype(kr.LD) - G)
    bad = mask & ~(err <= kr.LD(K) * E)
    if bad.any():
        p = int(np.flatnonzero(bad)[0])
        i, j = divmod(p, n1)
        pytest.fail(f"{case.id} [{path}]: {int(bad.sum())} of {int(mask.sum())} entries beyond K * E; first at (row, column) multi-index "
                    f"{case.describe(p)}: got {got[i, j]!r}, reference {float(G[i, j])!r}, envelope {float(E[i, j])!r}; "
                    f"worst ratio {ratio / kr.EPS:.2f} eps at {case.describe(pos)}")
    # nothing outside the block was written (the lower triangle is what `todense` reads; it mirrors it)
    outside = np.tril(np.ones(after.shape, dtype=bool))
    outside[r0:r0 + n0, c0:c0 + n1] = False
    assert np.array_equal(before.view(np.uint64)[outside], after.view(np.uint64)[outside]), f"{case.id}: a write outside the block"
