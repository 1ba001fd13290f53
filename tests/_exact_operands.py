"""Integer operands for the kernels that only multiply and add (csrc/trmm.hip, the contraction of csrc/evidence_grad.hip, the sum of
squares of csrc/evidence.hip): with small integers in every operand each product and each partial sum is an integer far below
2^53, so fp64 computes it exactly WHATEVER the order of summation -- the result of any launch shape, any chunk size and any
number of trips must equal the int64 reference bit for bit, and a term that is dropped, taken twice or read from a stale buffer
changes an integer.  Everything the kernels must not read holds NaN or 1e30.

The builders are plain NumPy (checked on the CPU in test_exact_operands.py); `identity_factored` and `cleared` are the two device
matrices the operands are written into through the hook `lpgp_test_mat_raw` (tests/_hooks.py mat_raw).  A plain module the suites
import, not a conftest."""
import numpy as np

TILE = 128
EXACT_LIMIT = 2 ** 53            # every integer of modulus up to here is an fp64 number


def padded(nb):
    return -(-nb // TILE) * TILE


def logical_mask(sizes):
    """Boolean mask over the padded rows of a matrix with blocks of `sizes` rows: True for a logical row, False for padding."""
    mask = np.zeros(sum(padded(nb) for nb in sizes), dtype=bool)
    off = 0
    for nb in sizes:
        mask[off:off + nb] = True
        off += padded(nb)
    return mask


def garbage(rng, shape):
    """NaN and 1e30, half each: what a masked position holds."""
    return np.where(rng.uniform(size=shape) < 0.5, np.nan, 1e30)


def trmm_operands(sizes, s, seed, lim=8):
    """Operands of `shift + tril(L) Z` for a factor in the layout of `sizes`:
      raw    the padded storage (pn x pn float64): integers of [-lim, lim] on and below the diagonal of the logical rows and columns, the
             identity's entries (1 on the diagonal, 0 beside it) in the padding rows and columns on and below the diagonal, NaN and 1e30
             everywhere above the diagonal -- inside the diagonal tiles and in the whole tiles above them;
      L      the logical lower triangle (n x n int64), Z (n x s int64), shift (n int64);
      ref    shift[:, None] + L @ Z in int64."""
    rng = np.random.default_rng(seed)
    mask = logical_mask(sizes)
    pn, n = mask.size, int(mask.sum())
    L = np.tril(rng.integers(-lim, lim + 1, (n, n)))
    low = np.eye(pn, dtype=np.int64)
    low[np.ix_(mask, mask)] = L
    raw = np.where(np.tril(np.ones((pn, pn), dtype=bool)), low.astype(np.float64), garbage(rng, (pn, pn)))
    Z = rng.integers(-lim, lim + 1, (n, s))
    shift = rng.integers(-lim, lim + 1, n)
    return raw, L, Z, shift, shift[:, None] + L @ Z


def trmm_partial_sum_bound(n, lim=8):
    """The largest modulus any partial sum of an entry of shift + tril(L) Z can reach, in any order of summation."""
    return n * lim * lim + lim


def contraction_operands(sizes, seed, lim=4):
    """Operands of the pair (w^T dG w, tr(G^-1 dG)) read from two lower triangles in the layout of `sizes`, with w = r (the factor is the
    identity):
      raw    {"ginv", "dG"}: the padded storages (pn x pn float64): integers of [-lim, lim] where row and column are logical and
             row >= column, NaN and 1e30 everywhere else (the padding rows and columns, everything above the diagonal);
      r      n integers (int64), v: n integers (the diagonal of the `_diag` form, over all logical rows);
      q, t   sum_ij f_ij r_i r_j dG_ij and sum_ij f_ij Ginv_ij dG_ij with f = 1 on the diagonal, 2 below it, in int64;
      diag   the logical diagonal of Ginv (int64)."""
    rng = np.random.default_rng(seed)
    mask = logical_mask(sizes)
    pn, n = mask.size, int(mask.sum())
    keep = np.tril(np.ones((pn, pn), dtype=bool)) & mask[:, None] & mask[None, :]
    raw, tri = {}, {}
    for name in ("ginv", "dG"):
        full = rng.integers(-lim, lim + 1, (pn, pn))
        raw[name] = np.where(keep, full.astype(np.float64), garbage(rng, (pn, pn)))
        tri[name] = np.where(keep, full, 0)[np.ix_(mask, mask)]
    r = rng.integers(-lim, lim + 1, n)
    v = rng.integers(-lim, lim + 1, n)
    f = 2 * np.tril(np.ones((n, n), dtype=np.int64), -1) + np.eye(n, dtype=np.int64)
    q = int(np.sum(f * np.outer(r, r) * tri["dG"]))
    t = int(np.sum(f * tri["ginv"] * tri["dG"]))
    return raw, r, v, q, t, np.diag(tri["ginv"]).copy()


def contraction_partial_sum_bound(n, lim=4):
    """The largest modulus a partial sum of either quantity can reach: n^2 terms of at most 2 lim^3."""
    return 2 * lim ** 3 * n * n


# ---- the two device matrices the operands go into (GPU) ----------------------------------------------------------------------
def cleared(ctx, sizes):
    """An unfactored device matrix with blocks of `sizes` rows, every block assembled from the zero kernel."""
    import linpde_gp_amd as lp
    from linpde_gp_amd import _engine
    zero = (0.0 * lp.randprocs.covfuncs.ExpQuad((1,), lengthscales=1.0)).lower()
    M = _engine.GramMatrix(ctx, sum(padded(nb) for nb in sizes))
    pts = []
    for i, nb in enumerate(sizes):
        P = _engine.Points(ctx, np.zeros((nb, 1)))
        M.add_block(nb)
        for j in range(i):
            M.assemble(zero, P, pts[j], i, j)
        M.assemble(zero, P, None, i, i)
        pts.append(P)
    return M


def identity_factored(ctx, sizes):
    """The identity, factored: zero kernel, `add_diag` 1, `potrf`.  Its state is that of any factored matrix; its storage may then be
    overwritten through `mat_raw`."""
    M = cleared(ctx, sizes)
    for i in range(len(sizes)):
        M.add_diag(i, scalar=1.0)
    assert M.potrf() == 0
    assert M.padded_n == sum(padded(nb) for nb in sizes) and M.n == sum(sizes)
    return M
