"""csrc/trmm.hip at every chunk size of its work split.  `factor_matmul` cuts tile row i of the staircase into chunks of at most
kc tiles of columns, one workgroup each, and picks kc in {8, 4, 2, 1} from the size and the CU count; a workgroup walks its chunk
through two LDS buffers of Z with one barrier per step.  On a 256-CU device the entrywise cases of test_gpu_sample.py get kc = 1 or 2;
only its draws with Z = I of 900 x 900 reach kc = 4 (through `sample()`, at a bar of 1e-9 on C C^T), and nothing reaches kc = 8, the
chunk size of the README's workloads: no chunk of more than four steps, no row whose full chunks of eight are followed by a short
last one that holds the diagonal tile, and no exact or entrywise check beyond two steps.  The hook `lpgp_test_factor_matmul`
(tests/_hooks.py) takes kc as an argument.

Exact operands (tests/_exact_operands.py, held on the CPU in test_exact_operands.py).  trmm.hip reads `mat->a` only, so a factored
matrix can be handed ANY lower triangle through `lpgp_test_mat_raw`: the identity is factored (zero kernel, `add_diag` 1, `potrf`)
and its storage overwritten with integers of [-8, 8] on and below the diagonal, NaN and 1e30 everywhere above it (inside the
diagonal tiles and in the whole tiles above them), the identity's entries in the padding rows and columns.  With Z and the shift
integers of [-8, 8] too, every partial sum is an integer below 2^17 (2^18 at 2500 rows): fp64 is exact in any order, and the result
must EQUAL `shift[:, None] + tril(L) @ Z` formed in int64, for every kc, with the same bits from every kc and from a second call.
A step that stages the wrong Z tile, a chunk dropped or added twice, a stale buffer, a diagonal tile unmasked: each changes an integer
(or lets a NaN in).

Layouts: one block of 1280 rows (T = 10 tile rows, no padding: with kc = 8 row 9 has a chunk of eight steps and one of two, with
kc = 4 every row from 4 on has several chunks and every full chunk four steps); one block of 1250 rows (a tail of 30 padding rows);
blocks of 130 + 300 + 700 rows (1408 padded rows, T = 11, padding between the blocks).  s = 1, 16, 17, 40: one column, one full
column tile, one column into the second, a ragged third.

Real operands: the device's own factor of an SPD matrix of 1250 rows, each kc against the long-double product at the entrywise
bound of test_gpu_sample.py, `(n + 2) u (|tril L| |Z| + |shift|)`, the bound of an inner product of length n in any order.

The public path, `mat.factor_matmul`, with exact operands at (n, s) = (1280, 1040) and (2500, 130), where a 256-CU device picks
kc = 8 and kc = 4 by the formula (12 chunks x 65 column tiles >= 512; 36 chunks of eight x 9 = 324 < 512 <= 60 chunks of four x 9).  The
assertion is equality whatever kc the device picks; the test does not re-derive kc.

Defect runs (recorded in MEASUREMENTS.md, not tests; scratch builds that stay in bounds).  Step j of trmm_lower_kernel staging the Z tile
of j0 + ((j - j0) & 1): 15 of the 16 tests here fail, from kc = 4 on (and 4 of the earlier suite's, the 900 x 900 draws).  Steps five to
eight of a chunk staging the tile of four steps earlier: everything the suite held before passes, 14 tests here fail, at kc = 8."""
import numpy as np
import pytest

import _exact_operands as ex
import _hooks

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KCS = (1, 2, 4, 8)
LAYOUTS = {"1280": (1280,), "1250": (1250,), "130+300+700": (130, 300, 700)}


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    yield _engine.default_context()
    _mats.clear()                   # (the matrices go while the library is still loaded)


_mats = {}


def integer_factor(ctx, name, sizes, seed):
    """The factored identity in the layout `sizes` with the integer lower triangle of `trmm_operands(sizes, ., seed)` written over its
    storage: made once per layout (the triangle does not depend on the number of columns)."""
    if name not in _mats:
        mat = ex.identity_factored(ctx, sizes)
        raw = ex.trmm_operands(sizes, 1, seed)[0]
        _hooks.mat_raw(ctx, mat, raw)
        back = _hooks.mat_raw(ctx, mat)
        assert back.tobytes() == np.ascontiguousarray(raw).tobytes()      # (NaN payloads included: the storage is what was written)
        _mats[name] = mat
    return _mats[name]


@pytest.mark.parametrize("s", [1, 16, 17, 40])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_chunk_size_is_exact_on_integer_operands(ctx, layout, s):
    sizes = LAYOUTS[layout]
    seed = 1000 + sum(sizes)
    mat = integer_factor(ctx, layout, sizes, seed)
    raw, L, Z, shift, ref = ex.trmm_operands(sizes, s, seed)
    n = L.shape[0]
    assert mat.n == n and mat.padded_n == raw.shape[0] and ex.trmm_partial_sum_bound(n) < 2 ** 17
    ref0 = L @ Z
    outs = {}
    for kc in KCS:
        out = _hooks.factor_matmul(ctx, mat, Z, shift, kc)
        bad = np.flatnonzero(~(out == ref).all(axis=1))
        print(f"trmm exact {layout} s={s} kc={kc}: {bad.size} of {n} rows differ" + (f", first at row {bad[0]} (tile row {bad[0] // 128})" if bad.size else ""))
        assert np.array_equal(out, ref), f"kc = {kc}: {bad.size} rows differ from the int64 product, first {bad[:8]}"
        assert np.array_equal(_hooks.factor_matmul(ctx, mat, Z, None, kc), ref0), f"kc = {kc}, no shift"
        assert _hooks.factor_matmul(ctx, mat, Z, shift, kc).tobytes() == out.tobytes(), f"kc = {kc}: a second call returns other bits"
        outs[kc] = out.tobytes()
    assert len(set(outs.values())) == 1, "the chunk sizes do not return the same bits"
    assert mat.factor_matmul(Z, shift).tobytes() == outs[1], "the public call returns other bits than the hook"


def test_the_hook_refuses_what_the_public_call_refuses(ctx):
    from linpde_gp_amd import _lib
    mat = integer_factor(ctx, "1250", LAYOUTS["1250"], 1000 + 1250)
    Z = np.ones((1250, 2))
    for kc in (0, 3, 16, -1):
        with pytest.raises(_lib.LpgpError, match="chunk size is 1, 2, 4 or 8"):
            _hooks.factor_matmul(ctx, mat, Z, None, kc)
    plain = ex.cleared(ctx, (8,))
    with pytest.raises(_lib.LpgpError, match=r"not \(fully\) factored"):
        _hooks.factor_matmul(ctx, plain, np.ones((8, 2)), None, 4)


def test_every_chunk_size_within_the_entrywise_bound_on_a_real_factor(ctx):
    """The device's own Cholesky factor of B B^T + n I at n = 1250 (the matrix `_factored_dense` of test_gpu_sample.py builds), s = 5
    and 17, with and without a shift: every kc within (n + 2) u (|tril L| |Z| + |shift|) of the long-double product."""
    import linpde_gp_amd as lp
    from linpde_gp_amd import _engine
    n = 1250
    rng = np.random.default_rng(100 + n)
    B = rng.standard_normal((n, n))
    A = B @ B.T + n * np.eye(n)
    mat = _engine.GramMatrix(ctx, n)
    bi = mat.add_block(n)
    mat.assemble(lp.randprocs.covfuncs.Zero(()).lower(), _engine.Points(ctx, np.zeros((n, 1))), None, bi, bi)
    mat.add_dense(bi, A)
    assert mat.potrf() == 0
    L = mat.todense("factor")
    Ll, aL = np.tril(L).astype(np.longdouble), np.abs(np.tril(L))
    top = 0.0
    for s in (5, 17):
        Z = rng.standard_normal((n, s))
        for shift in (None, rng.standard_normal(n) * 3.0):
            sh = np.zeros(n) if shift is None else shift
            ref = sh[:, None].astype(np.longdouble) + Ll @ Z.astype(np.longdouble)
            bound = (n + 2) * U * (aL @ np.abs(Z) + np.abs(sh)[:, None])
            for kc in KCS:
                out = _hooks.factor_matmul(ctx, mat, Z, shift, kc)
                err = np.abs(out.astype(np.longdouble) - ref)
                worst = float(np.max(err / np.maximum(bound, 1e-300)))
                top = max(top, worst)
                print(f"trmm real n={n} s={s} shift={shift is not None} kc={kc}: max err / bound = {worst:.3e}")
                assert np.all(err <= bound), (s, kc, worst)
                assert _hooks.factor_matmul(ctx, mat, Z, shift, kc).tobytes() == out.tobytes()
    print(f"trmm real n={n}: largest err / bound over all kc = {top:.3e}")


@pytest.mark.parametrize("n,s", [(1280, 1040), (2500, 130)])
def test_the_public_path_is_exact_where_it_picks_long_chunks(ctx, n, s):
    sizes = (n,)
    seed = 2000 + n
    mat = ex.identity_factored(ctx, sizes)
    raw, L, Z, shift, ref = ex.trmm_operands(sizes, s, seed)
    _hooks.mat_raw(ctx, mat, raw)
    assert ex.trmm_partial_sum_bound(n) < ex.EXACT_LIMIT
    out = mat.factor_matmul(Z, shift)
    bad = np.flatnonzero(~(out == ref).all(axis=1))
    print(f"trmm public n={n} s={s}: {bad.size} rows differ")
    assert np.array_equal(out, ref), f"{bad.size} rows differ from the int64 product, first {bad[:8]}"
    assert mat.factor_matmul(Z, shift).tobytes() == out.tobytes()
