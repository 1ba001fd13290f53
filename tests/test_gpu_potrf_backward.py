"""The blocked fp64 Cholesky (`lpgp_potrf`: csrc/potrf.hip, chain.hip, potrf_tile.h, gemm.hip, solve*) against LAPACK-level
accuracy on synthetic matrices, over the schedule options that select its branches.

Single blocks enter as a drop-in caller's do (`randvars/_normal.py`): the block cleared by the Zero kernel, then `add_dense`.
Three kinds (seeded):
  (a) B B^T / k + I, well conditioned;
  (b) the Gram of a 2-D Matern-5/2 on scattered points plus a nugget of 1e-8 (condition ~1e9 and more);
  (c) D A D, A of kind (a), D log-uniform over 1e-6 .. 1e6.
Appended block rows enter as a conditioning builds them: every block of the new row assembled by the device (a Matern-5/2
Gram), then the noise on the diagonal (`add_diag`); the reference is that same device-assembled matrix, read back unfactored.
The backward error is measured after the symmetric diagonal scaling S = diag(A)^{-1/2} -- max |S (A - L L^T) S| -- which
Cholesky keeps small whatever D is (an absolute threshold or a lost scale inside the factorisation shows on kind (c)).  It is
formed in long double: in full for n <= 512 and on `PROBES` random probe vectors above (the full product costs seconds of
host time per factor from n ~ 1000 on).  Every bar is relative to LAPACK (`np.linalg.cholesky`) on the same matrix and
probes, plus an absolute ceiling."""
import numpy as np
import pytest
import scipy.linalg

from _backward import EPS, LD, Appender, backward_error, gram_points, restored
from _backward import matern52 as _matern52, mv as _mv, scale as _scale

pytestmark = pytest.mark.gpu

# Bars, set from the first MI355X run (the largest measured value in brackets).  The device factor's backward error is a few
# times LAPACK's on the well-conditioned kinds (a), (c) [7.6 at n = 100, 6.0 at n = 8320] and below it on kind (b) [0.4]: at
# most 0.2 n eps in all.  Its solves: [4.8 x cho_solve's normwise backward error].
RATIO = 10.0                # factor: backward error <= RATIO x LAPACK's on the same matrix and probes
CEIL = 0.5                  # ... and <= CEIL * n * eps (scaled)
RATIO_SOLVE = 8.0

OPTIONS = ("nb", "lookahead", "chain_resident_max_rows", "chain_resident2_max_rows", "chain_ahead", "nb_outer", "nb_outer_min_tiles",
           "nb_big", "nb_big_min_tiles", "gemm3", "gemm3_fact", "small_tiles_max", "small_ring2", "dense_tiles", "fused_solve",
           "append_split")


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


@pytest.fixture
def sched(ctx):
    """sched(dict) applies a schedule row; every option of `OPTIONS` is restored afterwards, profiling switched off."""
    with restored(ctx, OPTIONS) as apply:
        yield apply


# ---- matrices (module cache: the host references dominate the cost) ----------------------------------------------------
_cache = {}


def matrix(kind, n):
    key = ("A", kind, n)
    if key not in _cache:
        rng = np.random.default_rng(1000 * n + ord(kind))
        if kind == "a":
            k = min(n, 256)
            B = rng.standard_normal((n, k))
            A = B @ B.T / k + np.eye(n)
        elif kind == "b":
            A = _matern52(n, rng)
        else:
            d = 10.0 ** rng.uniform(-6, 6, n)
            A = d[:, None] * matrix("a", n) * d[None, :]
        _cache[key] = np.ascontiguousarray((A + A.T) / 2)        # exactly symmetric
    return _cache[key]


def lapack(A):
    """(LAPACK's factor, its backward error) of a matrix held in the module cache."""
    key = ("L", id(A))
    if key not in _cache:
        L = np.linalg.cholesky(A)
        _cache[key] = (L, backward_error(A, L))
    return _cache[key]


# ---- upload ---------------------------------------------------------------------------------------------------------------
def new_matrix(ctx, A):
    """GramMatrix holding A as one block, not factored: the block cleared by the Zero kernel, then A added."""
    from linpde_gp_amd import _engine
    from linpde_gp_amd.randprocs import covfuncs
    n = A.shape[0]
    mat = _engine.GramMatrix(ctx, n)
    bi = mat.add_block(n)
    pts = _engine.Points(ctx, np.zeros((n, 1)))
    mat.assemble(covfuncs.Zero(()).lower(), pts, None, bi, bi)
    mat.add_dense(bi, A)
    return mat


def factor(ctx, A):
    mat = new_matrix(ctx, A)
    assert mat.potrf() == 0
    return mat


def appended_matrix(kind, n, blocks):
    """The device-assembled Gram of `blocks` (read back before any factorisation): the reference of the appended factors."""
    key = ("G", kind, n, tuple(blocks))
    if key not in _cache:
        from linpde_gp_amd import _engine
        ap = Appender(_engine.default_context(), *gram_points(kind, n))
        for nb in blocks:
            ap.add(nb)
        _cache[key] = ap.mat.todense("gram")
    return _cache[key]


def factor_appended(ctx, kind, n, blocks):
    ap = Appender(ctx, *gram_points(kind, n))
    for nb in blocks:
        ap.add(nb)
        assert ap.mat.potrf() == 0
    return ap


def check_factor(mat, A, tag):
    """The bars on a factored matrix; returns (backward error, ratio to LAPACK, L)."""
    n = A.shape[0]
    L = mat.todense("factor")
    assert np.all(np.triu(L, 1) == 0.0), tag
    assert np.array_equal(mat.factor_diag(), np.diag(L)), tag
    assert np.all(np.isfinite(L)), tag
    be = backward_error(A, L)
    be_ref = lapack(A)[1]
    ratio = be / max(be_ref, 1e-3 * EPS)
    print(f"\n[potrf {tag}] n={n} backward error {be:.3e} (LAPACK {be_ref:.3e}): ratio {ratio:.2f}, {be / (n * EPS):.3f} n eps")
    assert be <= RATIO * max(be_ref, 1e-3 * EPS), f"{tag}: backward error {be:.3e} > {RATIO} x LAPACK's {be_ref:.3e}"
    assert be <= CEIL * max(n, 8) * EPS, f"{tag}: backward error {be:.3e} > {CEIL} n eps"
    return be, ratio, L


def check_solves(mat, A, tag):
    n = A.shape[0]
    rng = np.random.default_rng(n + 17)
    Lref = lapack(A)[0]
    nA = float(np.max(np.sum(np.abs(A), axis=1)))
    for nrhs in (1, 9):
        b = rng.standard_normal((n, nrhs))
        out = []
        for x in (mat.potrs(b[:, 0] if nrhs == 1 else b).reshape(n, nrhs), scipy.linalg.cho_solve((Lref, True), b)):
            r = _mv(A, x.astype(LD)) - b.astype(LD)
            out.append(float(np.max(np.abs(r))) / (nA * float(np.max(np.abs(x))) + float(np.max(np.abs(b)))))
        ratio = out[0] / out[1]
        print(f"[potrs {tag}] nrhs={nrhs}: backward error {out[0]:.3e} (cho_solve {out[1]:.3e}): ratio {ratio:.2f}")
        assert out[0] <= RATIO_SOLVE * out[1], f"{tag} nrhs={nrhs}: {out[0]:.3e} vs cho_solve {out[1]:.3e}"


# ---- the default schedule over sizes and kinds ---------------------------------------------------------------------------
SIZES = [1, 100, 127, 128, 129, 511, 512, 513, 640, 1500, 2125, 4608]


@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("n", SIZES)
def test_default_schedule(ctx, kind, n):
    A = matrix(kind, n)
    mat = factor(ctx, A)
    check_factor(mat, A, f"default {kind}")
    if n in (513, 2125):
        check_solves(mat, A, f"default {kind} n={n}")


def test_default_schedule_c2_size(ctx):
    """8320 rows: c2's 65 tiles (a ragged last panel of one tile, nine panels behind the two-level threshold)."""
    A = matrix("a", 8320)
    check_factor(factor(ctx, A), A, "default a")


# ---- schedule rows ---------------------------------------------------------------------------------------------------------
# (id, options, sizes, profiling slots that must have launched (> 0) / must not have (== 0))
SCHEDULES = [
    # (launches small enough for the 64 x 64 kernel all count in slot gemm_small: rows that assert a slot of a triangular
    #  update set small_tiles_max = 0)
    ("defaults", {}, [2125, 4608], ["panel_fused"], []),
    ("lookahead0", {"lookahead": 0, "small_tiles_max": 0}, [513, 2125], ["syrk_trailing"], ["syrk_lookahead"]),
    ("nb256", {"nb": 256}, [513, 2125], [], []),
    ("nb1024", {"nb": 1024}, [2125, 4608], [], []),
    ("tile_by_tile_chain", {"chain_resident_max_rows": -1}, [513, 2125], ["potrf_tile", "trsm_gemm"], ["panel_fused"]),
    ("resident2", {"chain_resident_max_rows": 4, "chain_resident2_max_rows": 64}, [2125], ["panel_fused"], []),
    ("chain_ahead0", {"chain_ahead": 0, "small_tiles_max": 0}, [2125, 4608], ["panel_fused", "syrk_lookahead"], []),
    ("two_level_outer", {"nb_outer": 1024, "nb_outer_min_tiles": 0, "small_tiles_max": 0}, [2125, 4608],
     ["syrk_lookahead", "syrk_trailing"], []),
    ("nb_big", {"nb_big": 1024, "nb_big_min_tiles": 8}, [2125, 4608], [], []),
    ("gemm3_fact", {"gemm3": 1, "gemm3_fact": 1, "small_tiles_max": 0}, [1500, 4608], ["syrk_trailing"], ["gemm_small"]),
    ("small_tiles0", {"small_tiles_max": 0}, [513, 2125], ["syrk_lookahead"], ["gemm_small"]),
    ("small_tiles_all", {"small_tiles_max": 1 << 20}, [513, 2125], ["gemm_small"], ["syrk_trailing", "syrk_lookahead"]),
    ("small_ring2_off", {"small_ring2": 0, "chain_resident_max_rows": -1, "small_tiles_max": 1 << 20}, [2125], ["gemm_small"], []),
    ("small_ring2_1", {"small_ring2": 1, "chain_resident_max_rows": -1, "small_tiles_max": 1 << 20}, [2125], ["gemm_small"], []),
    ("dense_tiles0", {"dense_tiles": 0, "small_tiles_max": 0}, [2125, 4608], ["syrk_trailing"], []),
    ("fused_solve0", {"fused_solve": 0}, [2125], [], []),
]


@pytest.mark.parametrize("row", SCHEDULES, ids=[r[0] for r in SCHEDULES])
def test_schedule(ctx, sched, row):
    name, opts, sizes, must, must_not = row
    sched(opts)
    for n in sizes:
        A = matrix("b", n)
        ctx.profile_enable(True)
        ctx.profile_reset()
        mat = factor(ctx, A)
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        for slot in must:
            assert prof[slot]["launches"] > 0, f"{name} n={n}: no launch in slot {slot}: the row no longer selects its branch"
        for slot in must_not:
            assert prof[slot]["launches"] == 0, f"{name} n={n}: {prof[slot]['launches']} launches in slot {slot}"
        _, _, L = check_factor(mat, A, f"{name} b")
        if n == sizes[-1] or n == 2125:
            check_solves(mat, A, f"{name} n={n}")
        if n == sizes[0]:
            # run-to-run bit identity: no floating-point atomics anywhere in potrf / chain / gemm / solve
            L2 = factor(ctx, A).todense("factor")
            assert np.array_equal(L, L2), f"{name} n={n}: two factorisations of the same matrix differ"


# ---- appends -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["m", "b", "s"])
def test_appends(ctx, kind):
    """Blocks of 300, 77, 1, 513 and the rest of 2125 rows, each factored as it arrives: the same bars as one block, and
    the same factor as one block to LAPACK level."""
    n = 2125
    blocks = [300, 77, 1, 513, n - 891]
    A = appended_matrix(kind, n, blocks)
    mat = factor_appended(ctx, kind, n, blocks).mat
    _, _, L = check_factor(mat, A, f"append {kind}")
    check_solves(mat, A, f"append {kind}")
    L1 = factor(ctx, A).todense("factor")
    s = _scale(A)
    d_dev, d_lap = np.max(np.abs((L - L1) * s[:, None])), np.max(np.abs((lapack(A)[0] - L1) * s[:, None]))
    print(f"[append {kind}] |L_append - L_one| = {d_dev:.3e}, |L_lapack - L_one| = {d_lap:.3e} (row-scaled)")
    assert d_dev <= RATIO * max(d_lap, EPS)


@pytest.mark.parametrize("opts", [{"append_split": 1, "small_tiles_max": 0}, {"fused_solve": 0}, {"lookahead": 0}],
                         ids=["append_split", "fused_solve0", "lookahead0"])
def test_append_schedules(ctx, sched, opts):
    """A new block of >= 16 tile rows behind an old one (append_split: the last old panel's update split, slot syrk_lookahead)."""
    sched(opts)
    n, blocks = 3113, [513, 2600]
    A = appended_matrix("b", n, blocks)
    ap = Appender(ctx, *gram_points("b", n))
    ap.add(blocks[0])
    assert ap.mat.potrf() == 0
    ap.add(blocks[1])
    ctx.profile_enable(True)
    ctx.profile_reset()
    assert ap.mat.potrf() == 0
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    if opts.get("fused_solve", 1):
        assert prof["panel_fused"]["launches"] > 0
    if opts.get("append_split"):
        assert prof["syrk_lookahead"]["launches"] > 0
    check_factor(ap.mat, A, f"append {list(opts)[0]} b")
    check_solves(ap.mat, A, f"append {list(opts)[0]}")


# ---- first bad pivot -----------------------------------------------------------------------------------------------------
PIV_N = 2125


def pivot_positions(ctx):
    nb = ctx.get_option("nb")
    ragged = (PIV_N // 128) * 128 + 1
    return sorted({1, 2, 128, 129, 512, 513, nb + 1, 2 * nb + 1, ragged, PIV_N})


def broken(A, L, k):
    """A with the k-th (1-based) pivot made -delta (delta = A_kk / 2); the leading minors before k are unchanged."""
    B = A.copy()
    d = 0.5 * A[k - 1, k - 1]
    B[k - 1, k - 1] -= L[k - 1, k - 1] ** 2 + d
    return B


SCHED_PIV = [r for r in SCHEDULES if r[0] not in ("small_ring2_off", "fused_solve0")]


@pytest.mark.parametrize("row", SCHED_PIV, ids=[r[0] for r in SCHED_PIV])
def test_first_bad_pivot(ctx, sched, row):
    """info names the first pivot that is not positive, exactly, on every schedule row; eagerly (`potrf`) and enqueued
    (`potrf_enqueue` + `check`, which names the block too); after it the block is dropped and a corrected one factors."""
    sched(row[1])
    A = matrix("a", PIV_N)
    L = lapack(A)[0]
    for k in pivot_positions(ctx):
        B = broken(A, L, k)
        mat = new_matrix(ctx, B)
        assert mat.potrf() == k, f"{row[0]}: eager potrf, pivot {k}"
        mat.pop_block()
        mat2 = new_matrix(ctx, B)
        mat2.potrf_enqueue()
        assert mat2.check() == (k, 0), f"{row[0]}: enqueued potrf, pivot {k}"
        mat2.truncate(0)
    # a corrected block then factors in the matrix that failed
    from linpde_gp_amd.randprocs import covfuncs
    from linpde_gp_amd import _engine
    bi = mat.add_block(PIV_N)
    mat.assemble(covfuncs.Zero(()).lower(), _engine.Points(ctx, np.zeros((PIV_N, 1))), None, bi, bi)
    mat.add_dense(bi, A)
    assert mat.potrf() == 0
    check_factor(mat, A, f"after failure {row[0]} a")


def test_a_status_goes_to_the_word_of_its_own_factorisation(ctx):
    """An enqueued factorisation reports to its matrix's sticky word, an eager one to the caller, whatever other factorisation
    ran in between on the same context (pivot 129: the first of the second tile, inside the first resident panel)."""
    k = 129
    A = matrix("a", PIV_N)
    B = broken(A, lapack(A)[0], k)
    bad = new_matrix(ctx, B)
    bad.potrf_enqueue()
    good = new_matrix(ctx, A)
    assert good.potrf() == 0
    assert bad.check() == (k, 0)
    # the other way round
    good2, bad2 = new_matrix(ctx, A), new_matrix(ctx, B)
    good2.potrf_enqueue()
    assert bad2.potrf() == k
    assert good2.check() == (0, -1)            # (lpgp_mat_check: no pivot failed, so no block is named)
    check_factor(good2, A, "enqueued, a failing factorisation behind it a")


@pytest.mark.parametrize("enqueue", [False, True], ids=["eager", "enqueued"])
def test_first_bad_pivot_in_an_appended_block(ctx, enqueue):
    """info counts the PADDED order: row j (0-based) of block b fails as poff(b) + j + 1; the old factor stays bitwise as it
    was, and a corrected block then factors.  (The pivot is broken through the new block's diagonal noise.)"""
    blocks = [300, 77, PIV_N - 377]            # padded offsets 0, 384, 512
    A = appended_matrix("m", PIV_N, blocks)
    L = lapack(A)[0]
    ap = Appender(ctx, *gram_points("m", PIV_N))
    for nb in blocks[:2]:
        ap.add(nb)
        assert ap.mat.potrf() == 0
    L_old = ap.mat.todense("factor")
    for j in (0, 1, 127, 128, 700, PIV_N - 378):
        k = 377 + j + 1
        extra = np.zeros(blocks[2])
        extra[j] = -(L[k - 1, k - 1] ** 2 + 0.5 * A[k - 1, k - 1])       # pivot k becomes -A_kk / 2
        ap.add(blocks[2], extra)
        if enqueue:
            ap.mat.potrf_enqueue()
            assert ap.mat.check() == (512 + j + 1, 2)
        else:
            assert ap.mat.potrf() == 512 + j + 1
        ap.drop(2, truncate=enqueue)
        assert np.array_equal(ap.mat.todense("factor"), L_old), f"row {j}: the old factor changed"
    ap.add(blocks[2])
    assert ap.mat.potrf() == 0
    check_factor(ap.mat, A, "after failure in block 2 m")


@pytest.mark.parametrize("what,k", [(w, k) for w in ("nan_diag", "inf_diag", "nan_below") for k in (1, 129, 513, PIV_N)
                                    if (w, k) != ("nan_below", 1)])           # (no entry left of the first pivot)
def test_nonfinite_entries(ctx, what, k):
    """NaN or Inf on the diagonal fails at that pivot; NaN below the diagonal at (k-1, j) fails at pivot k (the first whose
    computation reads it).  (LAPACK's dpotrf tests `ajj <= 0 or NaN` only: an Inf pivot passes there and the failure -- if
    any -- is reported one pivot later.  Here L's diagonal must be finite: see `test_huge_pivots`.)"""
    A = matrix("a", PIV_N).copy()
    if what == "nan_diag":
        A[k - 1, k - 1] = np.nan
    elif what == "inf_diag":
        A[k - 1, k - 1] = np.inf
    else:
        A[k - 1, k // 2] = A[k // 2, k - 1] = np.nan
    mat = new_matrix(ctx, A)
    assert mat.potrf() == k


def test_huge_pivots(ctx):
    """potrf_tile.h rejects a pivot whose square root -- L's diagonal entry -- is not in (0, 1e300): NaN and Inf
    (`test_nonfinite_entries`).  A finite pivot cannot reach the upper bound (sqrt(DBL_MAX) ~ 1.3e154), so diagonals up to
    1e300 factor as LAPACK factors them."""
    n = 640
    A = matrix("a", n).copy()
    big = [0, 200, 513, n - 1]
    for i, v in zip(big, [1e300, 1e250, 1e306, 1e300]):
        A[i, i] = v
    mat = new_matrix(ctx, A)
    assert mat.potrf() == 0
    L = mat.todense("factor")
    Lref = np.linalg.cholesky(A)
    np.testing.assert_allclose(np.diag(L), np.diag(Lref), rtol=1e-13)
    s = _scale(A)
    assert np.max(np.abs((L - Lref) * s[:, None])) <= 1e-12
