"""Every GEMM / SYRK kernel of csrc/gemm.hip against EXACT results, through the raw hook (`lpgp_test_gemm`).

Operands are integers in [-2^10, 2^10] and k <= 4096, so every product and every partial sum is an integer below 2^33: any
summation order gives the same float64 number.  The kernels start their accumulators from (beta / alpha) C and multiply by
alpha at the end, so the result is exact -- and must equal beta C0 + alpha A B formed on the host BIT FOR BIT -- whenever
beta / alpha is a power of two times a small integer (the (alpha, beta) pairs of `AB_EXACT`).  Other pairs (beta / alpha = 1/3)
are held to a forward-error bound against a long-double product in `test_gemm_random_operands_error_bound`.

Each launch embeds its operands in larger buffers: A and B carry NaN rows below their logical rows (a read with the wrong
stride turns into NaN in C), C carries sentinel rows that must come back bitwise unchanged, and for the triangular modes the
tiles above the diagonal must come back unchanged too.  Each row of `CASES` names the dispatch rule of `launch_gemm` /
`launch_small` / `pick_kernel` / `launch_impl` it satisfies."""
import numpy as np
import pytest

import _hooks      # tests/_hooks.py: liblpgp_testhooks.so (include/lpgp_test.h)

pytestmark = pytest.mark.gpu

T = 128
OPTIONS = ("small_tiles_max", "gemm3", "gemm3_fact", "small_ring2", "dense_tiles", "min_supertiles")
# (alpha, beta) with beta / alpha exact: the device result is exact
AB_EXACT = [(1.0, 1.0), (-1.0, 1.0), (0.5, -1.5), (-1.5, -1.5), (-1.5, 0.0), (1.0, 0.5), (-1.0, -1.5), (0.5, 0.0)]
SENTINEL = -7.0e21


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


@pytest.fixture
def opts(ctx):
    """set(**options) for one launch; every option of `OPTIONS` is restored afterwards."""
    saved = {k: ctx.get_option(k) for k in OPTIONS}

    def setter(**kw):
        for k, v in kw.items():
            assert k in OPTIONS
            ctx.set_option(k, v)
    try:
        yield setter
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def _ints(rng, shape):
    return rng.integers(-1024, 1025, size=shape).astype(np.float64)


def _valid_tiles(mt, nt, tri):
    return nt * (nt + 1) // 2 + (mt - nt) * nt if tri else mt * nt


def run_case(ctx, ta, tb, tri, mt, nt, k, alpha, beta, seed, pad=(8, 136, 8), exact=True, ints=True):
    """One launch on guarded buffers; returns (device C, reference C, C0) on the logical m x n region after checking the
    guards.  exact: bitwise equality on the written region, else the caller compares."""
    rng = np.random.default_rng(seed)
    m, n = mt * T, nt * T
    gen = (lambda s: _ints(rng, s)) if ints else (lambda s: rng.standard_normal(s))
    Am, Bm = gen((m, k)), gen((k, n))
    C0 = gen((m, n))
    if beta == 0.0:
        C0[:] = np.nan                                   # beta = 0: C is not read
    pa, pb, pc = pad
    a_rows, a_cols = (k, m) if ta else (m, k)            # ta: k fastest
    b_rows, b_cols = (k, n) if tb else (n, k)            # tb = 0: n fastest
    Abuf = np.full((a_rows + pa, a_cols), np.nan, order="F")
    Abuf[:a_rows] = Am.T if ta else Am
    Bbuf = np.full((b_rows + pb, b_cols), np.nan, order="F")
    Bbuf[:b_rows] = Bm if tb else Bm.T
    Cbuf = np.full((m + pc, n), SENTINEL, order="F")
    Cbuf[:m] = C0
    out, _ = _hooks.test_gemm(ctx, ta, tb, tri, alpha, Abuf, Bbuf, beta, Cbuf, k, m=m, n=n)
    assert np.array_equal(out[m:], Cbuf[m:]), "rows of C below m were written"
    C = out[:m]
    if ints:
        ref = alpha * (Am @ Bm) + (beta * C0 if beta != 0.0 else 0.0)
    else:
        ref = None
    if tri:
        # tiles strictly above the (128-tile) diagonal: untouched; inside a diagonal tile the kernel may write the part above the
        # diagonal (128 x 128 kernels) or not (64 x 64 kernel): either bitwise unchanged or the result there
        tr = np.arange(m)[:, None] // T
        tc = np.arange(n)[None, :] // T
        above = tr < tc
        assert np.array_equal(C[np.broadcast_to(above, C.shape)], C0[np.broadcast_to(above, C.shape)], equal_nan=True), \
            "a tile above the diagonal was written"
        if ref is not None:
            diag_upper = (tr == tc) & (np.arange(m)[:, None] < np.arange(n)[None, :])
            du = np.broadcast_to(diag_upper, C.shape)
            same_old = (C[du] == C0[du]) | (np.isnan(C[du]) & np.isnan(C0[du]))
            assert np.all(same_old | (C[du] == ref[du])), "upper part of a diagonal tile is neither old C nor the result"
    if exact and ref is not None:
        lower = np.broadcast_to(np.arange(m)[:, None] >= np.arange(n)[None, :], C.shape) if tri else np.ones(C.shape, bool)
        bad = ~(C[lower] == ref[lower])
        if np.any(bad):
            idx = np.argwhere(lower & ~(C == ref))[:5]
            raise AssertionError(f"{int(bad.sum())} of {int(lower.sum())} entries differ from the exact result; first at "
                                 f"{idx.tolist()}: device {C[tuple(idx[0])]!r}, exact {ref[tuple(idx[0])]!r}")
    return C, ref, C0, Am, Bm


# (id, ta, tb, tri, mt, nt, k, options): tile counts via _valid_tiles
CASES = [
    # ---- gemm64_f64_kernel<.., SS = 4> (launch_gemm: valid tiles <= small_tiles_max = 256 -> launch_small) ----
    ("small-nn-3x2-k48", 0, 0, 0, 3, 2, 48, {}),
    ("small-nt-3x2-k48", 0, 1, 0, 3, 2, 48, {}),
    ("small-tn-3x2-k48", 1, 0, 0, 3, 2, 48, {}),
    ("small-tt-3x2-k48", 1, 1, 0, 3, 2, 48, {}),
    ("small-1x1-k16", 0, 0, 0, 1, 1, 16, {}),
    ("small-tri1-6x6-k528", 0, 0, 1, 6, 6, 528, {}),
    ("small-tri3-9x4-k144", 0, 0, 3, 9, 4, 144, {}),          # (tri = 3 takes the TRI = 1 instantiation of launch_small)
    ("small-tri1-1x1-k16", 0, 0, 1, 1, 1, 16, {}),
    ("small-nn-16x16-k32-256tiles", 0, 0, 0, 16, 16, 32, {}),  # 256 tiles == small_tiles_max: still small
    ("small-tri1-256x1-k16-256tiles", 0, 0, 1, 256, 1, 16, {}),
    # tri = 2: k <= 128 and mt * nt >= small_ring2 (32) -> the two-stage ring SS = 2; below it, or k > 128, SS = 4
    ("small-tri2-31x1-k128-ss4", 0, 0, 2, 31, 1, 128, {}),
    ("small-tri2-32x1-k128-ss2", 0, 0, 2, 32, 1, 128, {}),
    ("small-tri2-8x4-k16-ss2", 0, 0, 2, 8, 4, 16, {}),
    ("small-tri2-8x4-k144-ss4", 0, 0, 2, 8, 4, 144, {}),
    ("small-tri2-8x4-k32-ring2off", 0, 0, 2, 8, 4, 32, {"small_ring2": 0}),
    # ---- gemm_f64_kernel, dense tile list (small_tiles_max = 0; gemm3 = 0): bands of 8 tile rows, band_prefix ----
    ("dense-nn-1x1-k16", 0, 0, 0, 1, 1, 16, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-nn-9x3-k144", 0, 0, 0, 9, 3, 144, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-nt-17x2-k32", 0, 1, 0, 17, 2, 32, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tn-7x3-k528", 1, 0, 0, 7, 3, 528, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tt-8x5-k48", 1, 1, 0, 8, 5, 48, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tri1-7x7-k128", 0, 0, 1, 7, 7, 128, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tri1-8x8-k16", 0, 0, 1, 8, 8, 16, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tri1-9x9-k2064", 0, 0, 1, 9, 9, 2064, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tri1-17x17-k48", 0, 0, 1, 17, 17, 48, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tri1-19x5-k144", 0, 0, 1, 19, 5, 144, {"small_tiles_max": 0, "gemm3": 0}),   # trapezoid, ragged last band
    ("dense-tri2-17x17-k128", 0, 0, 2, 17, 17, 128, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tri3-9x9-k528", 0, 0, 3, 9, 9, 528, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tri3-19x5-k32", 0, 0, 3, 19, 5, 32, {"small_tiles_max": 0, "gemm3": 0}),
    ("dense-tri1-40x40-k16", 0, 0, 1, 40, 40, 16, {}),          # 820 tiles: not small, gemm3_fact = 0 -> gemm_f64_kernel
    ("dense-tri2-40x40-k16", 0, 0, 2, 40, 40, 16, {}),
    ("dense-nn-257x1-k16-257tiles", 0, 0, 0, 257, 1, 16, {}),   # 257 tiles: one past small_tiles_max
    ("dense-tri1-257x1-k16-257tiles", 0, 0, 1, 257, 1, 16, {}),
    ("dense-nn-59x13-k32-767tiles", 0, 0, 0, 59, 13, 32, {}),   # 767 tiles: one below gemm3 = 768
    ("dense-tri1-256x3-k16-765tiles", 0, 0, 1, 256, 3, 16, {"gemm3_fact": 1}),   # below gemm3 even with gemm3_fact
    ("dense-tn-48x16-k32-768tiles", 1, 0, 0, 48, 16, 32, {}),   # 768 tiles but ta = 1: pick_kernel keeps gemm_f64_kernel
    # ---- gemm3_f64_kernel (pick_kernel: ta = 0, not tri = 2, tiles >= gemm3, and tri != 0 only with gemm3_fact) ----
    ("gemm3-nn-48x16-k32-768tiles", 0, 0, 0, 48, 16, 32, {}),
    ("gemm3-nt-48x16-k48-768tiles", 0, 1, 0, 48, 16, 48, {}),
    ("gemm3-nn-9x3-k144", 0, 0, 0, 9, 3, 144, {"small_tiles_max": 0, "gemm3": 1}),
    ("gemm3-nt-1x1-k528", 0, 1, 0, 1, 1, 528, {"small_tiles_max": 0, "gemm3": 1}),
    ("gemm3-tri1-17x17-k528", 0, 0, 1, 17, 17, 528, {"small_tiles_max": 0, "gemm3": 1, "gemm3_fact": 1}),
    ("gemm3-tri3-19x5-k2064", 0, 0, 3, 19, 5, 2064, {"small_tiles_max": 0, "gemm3": 1, "gemm3_fact": 1}),
    ("gemm3-tri1-257x3-k16-768tiles", 0, 0, 1, 257, 3, 16, {"gemm3_fact": 1}),
    ("gemm3-tri1-9x9-k16-fact0", 0, 0, 1, 9, 9, 16, {"small_tiles_max": 0, "gemm3": 1}),   # gemm3_fact = 0: gemm_f64_kernel
    # ---- super-tile mapping (dense_tiles = 0): map_tile with sshift from the first S in 8, 4, 2, 1 that gives at least
    #      min_supertiles super-tiles.  19 x 13 tiles: 6 / 20 / 70 / 247 super-tiles (full), 5 / 14 / 49 / 169 (lower) ----
    ("super-nn-19x13-sh3", 0, 0, 0, 19, 13, 32, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 1}),
    ("super-nn-19x13-sh2", 0, 0, 0, 19, 13, 32, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 20}),
    ("super-tn-19x13-sh1", 1, 0, 0, 19, 13, 32, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 70}),
    ("super-nt-19x13-sh0", 0, 1, 0, 19, 13, 48, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 1 << 20}),
    ("super-tri1-19x13-sh3", 0, 0, 1, 19, 13, 16, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 1}),
    ("super-tri1-19x13-sh2", 0, 0, 1, 19, 13, 16, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 14}),
    ("super-tri3-19x13-sh1", 0, 0, 3, 19, 13, 144, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 49}),
    ("super-tri2-19x13-sh0", 0, 0, 2, 19, 13, 16, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 1 << 20}),
    ("super-gemm3-tri1-19x13-sh1", 0, 0, 1, 19, 13, 32, {"small_tiles_max": 0, "gemm3": 1, "gemm3_fact": 1, "dense_tiles": 0,
                                                          "min_supertiles": 49}),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gemm_exact(ctx, opts, case):
    name, ta, tb, tri, mt, nt, k, o = case
    opts(**o)
    alpha, beta = AB_EXACT[sum(map(ord, name)) % len(AB_EXACT)]
    run_case(ctx, ta, tb, tri, mt, nt, k, alpha, beta, seed=sum(map(ord, name)))


@pytest.mark.parametrize("tri", [0, 1])
def test_gemm_exact_beyond_the_dense_band_table(ctx, opts, tri):
    """mt = 1537 tile rows, one band more than GemmArgs::MAXB = 192 bands of 8: launch_impl falls back to the super-tile
    mapping (C is 196 736 x 128, 200 MB)."""
    opts(min_supertiles=128)
    run_case(ctx, 0, 0, tri, 1537, 1, 16, -1.0, 1.0, seed=1537 + tri)


@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("beta", [1.0, -1.5, 0.0])
def test_gemm_alpha_zero(ctx, opts, tri, beta):
    """alpha = 0: C <- beta C (zeros for beta = 0, whatever C held) and A, B not read (BLAS).  The kernels scale C by
    beta / alpha on load: before the launch handled alpha = 0 itself, every entry came back NaN."""
    for o in ({"small_tiles_max": 0, "gemm3": 0}, {"small_tiles_max": 1 << 20}, {"small_tiles_max": 0, "gemm3": 1, "gemm3_fact": 1}):
        opts(**o)
        rng = np.random.default_rng(3)
        m, n, k = 5 * T, 3 * T, 32
        A = np.full((m, k), np.nan, order="F")
        B = np.full((n, k), np.nan, order="F")
        C0 = _ints(rng, (m, n))
        out, _ = _hooks.test_gemm(ctx, 0, 0, tri, 0.0, A, B, beta, C0, k)
        tr, tc = np.arange(m)[:, None] // T, np.arange(n)[None, :] // T
        written = np.broadcast_to((tr >= tc) if tri else True, C0.shape)
        assert np.array_equal(out[written], beta * C0[written]), o
        assert np.array_equal(out[~written], C0[~written]), o


def test_gemm_alpha_zero_public(ctx):
    """The same through the product's host GEMM (`_engine.gemm`, the dense products of `randvars/_normal.py`)."""
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(5)
    A, B, C0 = rng.standard_normal((300, 40)), rng.standard_normal((40, 200)), rng.standard_normal((300, 200))
    assert np.array_equal(_engine.gemm(ctx, A, B, alpha=0.0, beta=-1.5, C=C0), -1.5 * C0)
    assert np.array_equal(_engine.gemm(ctx, A, B, alpha=0.0, beta=0.0), np.zeros((300, 200)))


FLOAT_CASES = [
    # (id, ta, tb, tri, mt, nt, k, options, alpha, beta): beta / alpha = -1/3 is not exact -- the scaling of C rounds once
    ("small-nt", 0, 1, 0, 3, 2, 528, {}, -1.5, 0.5),
    ("small-tri2-ss2", 0, 0, 2, 32, 1, 128, {}, -1.0, 1.0),
    ("dense-tn", 1, 0, 0, 9, 2, 2064, {"small_tiles_max": 0, "gemm3": 0}, -1.5, 0.5),
    ("dense-tri1", 0, 0, 1, 9, 9, 528, {"small_tiles_max": 0, "gemm3": 0}, -1.0, 1.0),
    ("gemm3-nn", 0, 0, 0, 9, 3, 4096, {"small_tiles_max": 0, "gemm3": 1}, 0.5, -1.5),
    ("gemm3-tri3", 0, 0, 3, 9, 5, 528, {"small_tiles_max": 0, "gemm3": 1, "gemm3_fact": 1}, -1.5, 1.0),
    ("super-tt", 1, 1, 0, 9, 3, 144, {"small_tiles_max": 0, "gemm3": 0, "dense_tiles": 0, "min_supertiles": 20}, -1.5, 0.5),
]


@pytest.mark.parametrize("case", FLOAT_CASES, ids=[c[0] for c in FLOAT_CASES])
def test_gemm_random_operands_error_bound(ctx, opts, case):
    """Random float operands against a long-double product: |C - ref| <= gamma_{k+2} (|alpha| |A| |B| + |beta| |C0|), the
    bound of a recursive sum of k products started from the rounded (beta / alpha) C0 and scaled by alpha once."""
    name, ta, tb, tri, mt, nt, k, o, alpha, beta = case
    opts(**o)
    C, _, C0, Am, Bm = run_case(ctx, ta, tb, tri, mt, nt, k, alpha, beta, seed=sum(map(ord, name)), exact=False, ints=False)
    L = np.longdouble
    ref = L(alpha) * (Am.astype(L) @ Bm.astype(L)) + L(beta) * C0.astype(L)
    u = 2.0 ** -53
    gam = (k + 2) * u / (1 - (k + 2) * u)
    bound = gam * (abs(alpha) * (np.abs(Am) @ np.abs(Bm)) + abs(beta) * np.abs(C0))
    err = np.abs(C.astype(L) - ref).astype(np.float64)
    mask = (np.arange(C.shape[0])[:, None] >= np.arange(C.shape[1])[None, :]) if tri else np.ones(C.shape, bool)
    ratio = float(np.max(err[mask] / bound[mask]))
    print(f"\n[gemm {name}] max error / gamma bound = {ratio:.3e}")
    assert ratio <= 1.0
    assert ratio > 0.0 or k <= 16         # (a bound that is never approached would not be testing anything)
