"""The block-cyclic mode of the trailing update (csrc/gemm.hip: GemmArgs::cyc -- stair_nc / stair_decode inside map_tile_dense<TRI>,
the aidx / bidx arithmetic into the gathered panel in both 128 x 128 kernel bodies) against EXACT results, one rank at a time in this
process, through `lpgp_test_gemm_cyc`: the hook builds its launch arguments with the function potrf_dist uses (update_args,
csrc/dist.hip) and launches through launch_gemm.  In the manner of tests/test_gpu_gemm_exact.py.

Operands are integers in [-2^10, 2^10] and k <= 512, so every partial sum is an integer below 2^30 and the result is exact in any
summation order; with (alpha, beta) = (-1, 1) -- the product's pair -- or another pair of `AB_EXACT` the device result must equal
beta C0 + alpha P[gr - g0] P[gc - g0]^T BIT FOR BIT on every local tile (global (gr, gc)) with gr >= row_lo, col_lo <= gc < col_hi and
gr >= gc, and every other entry of the rank's storage must come back bitwise unchanged (inside a tile with gr == gc an entry above
the diagonal may hold the old value or the result: the rule of test_gpu_gemm_exact.py).  The storage carries sentinel rows below,
the panel NaN rows below its logical rows.  The reference (tests/_cyc_reference.py) restates the layout by brute force over global
tiles; tests/test_cyc_reference.py ties it to the host replay of the enumeration.

`gemm_band` is not an init-only option (csrc/options.cpp): set_option takes 4 / 8 / 16 and launch_impl reads it per launch.
The file's 42 cases -- some 3400 launches -- take about 10 s on an MI355X.
(Checked once against a broken kernel: with bidx = aidx in the body of gemm3_f64_kernel every case fails at its first gemm3 launch.)
The cyclic launches never take the 64 x 64 kernel (launch_gemm: `small` excludes cyc), so small_tiles_max stays at its default."""
import numpy as np
import pytest

import _cyc_reference as cr
import _hooks
from test_gpu_gemm_exact import AB_EXACT, SENTINEL

pytestmark = pytest.mark.gpu

T128 = cr.TILE
OPTIONS = ("gemm3", "gemm3_fact", "gemm_band")
PAD_P, PAD_C = 8, 8


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


@pytest.fixture
def restored(ctx):
    saved = {k: ctx.get_option(k) for k in OPTIONS}
    try:
        yield
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def _ints(rng, shape):
    return rng.integers(-1024, 1025, size=shape).astype(np.float64)


def test_scalar_pairs_are_exact_ones():
    assert cr.AB_PRODUCT in AB_EXACT and cr.AB_OTHER in AB_EXACT and cr.AB_OTHER != cr.AB_PRODUCT


@pytest.mark.parametrize("T", cr.TS)
@pytest.mark.parametrize("nbt", cr.NBTS)
@pytest.mark.parametrize("grid", cr.GRIDS, ids=[f"{a}x{b}" for a, b in cr.GRIDS])
def test_cyclic_update_exact(ctx, restored, grid, nbt, T):
    pr, pc = grid
    rng = np.random.default_rng(1000 * pr + 100 * pc + 10 * nbt + T)
    panels = {}                      # (g0, kt) -> (buffer with NaN rows below, P P^T): shared by the ranks and the launches
    stor = {}                        # rank -> (C0 buffer with sentinel rows, logical rows, logical columns)
    launches = written = 0
    for case in cr.cases(nbt, T):
        for k, v in case.opts.items():
            ctx.set_option(k, v)
        key = (case.g0, case.kt)
        if key not in panels:
            rows = (T - case.g0) * T128
            buf = np.full((rows + PAD_P, case.kt * T128), np.nan, order="F")
            buf[:rows] = _ints(rng, (rows, case.kt * T128))
            panels[key] = (buf, buf[:rows] @ buf[:rows].T)
        pbuf, PPt = panels[key]
        alpha, beta = case.ab
        for r in range(pr):
            for c in range(pc):
                if (r, c) not in stor:
                    m, n = len(cr.owned(pr, r, nbt, T)) * T128, len(cr.owned(pc, c, nbt, T)) * T128
                    C0 = np.full((m + PAD_C, n), SENTINEL, order="F")
                    C0[:m] = _ints(rng, (m, n))
                    stor[(r, c)] = (C0, m, n)
                C0, m, n = stor[(r, c)]
                out = _hooks.test_gemm_cyc(ctx, grid, (r, c), nbt, T, case.row_lo, case.col_lo, case.col_hi, case.g0, case.kt * T128,
                                           case.tri, case.occ3, alpha, beta, pbuf, C0)
                launches += 1
                where = (grid, (r, c), nbt, T, case)
                assert np.array_equal(out[m:], C0[m:]), ("rows below the rank's storage were written", where)
                pl = cr.plan(pr, pc, r, c, nbt, T, case)
                written += len(pl)
                ref = cr.apply_plan(pl, PPt, C0[:m], alpha, beta)
                got = out[:m]
                if np.array_equal(got, ref):
                    continue
                # not identical everywhere: the only freedom is the part above the diagonal of a tile with gr == gc
                rows, cols = cr.owned(pr, r, nbt, T), cr.owned(pc, c, nbt, T)
                free = np.zeros(got.shape, bool)
                for (lr, lc) in pl:
                    if rows[lr] == cols[lc]:
                        free[lr * T128:(lr + 1) * T128, lc * T128:(lc + 1) * T128] = np.triu(np.ones((T128, T128), bool), 1)
                bad = (got != ref) & ~free
                if np.any(bad):
                    i, j = np.argwhere(bad)[0]
                    raise AssertionError(f"{int(bad.sum())} entries differ from the exact result; first in local tile ({i // T128}, {j // T128}) "
                                         f"= global ({rows[i // T128]}, {cols[j // T128]}), planned: {(i // T128, j // T128) in pl}; device "
                                         f"{got[i, j]!r}, exact {ref[i, j]!r}, before {C0[i, j]!r}; {where}")
                old = C0[:m]
                assert np.all((got[free] == ref[free]) | (got[free] == old[free])), ("upper part of a diagonal tile is neither old nor result", where)
    assert launches == len(cr.cases(nbt, T)) * pr * pc and written > 0
