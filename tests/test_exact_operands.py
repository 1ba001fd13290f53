"""tests/_exact_operands.py on the CPU: the integer operands keep every partial sum an fp64 integer, so the float64 evaluation --
in NumPy's order, in a reversed order, in a chunked order -- equals the int64 reference bit for bit; the garbage sits exactly
where the kernels must not read.  No GPU."""
import numpy as np
import pytest

import _exact_operands as ex


def test_logical_mask_and_padding():
    m = ex.logical_mask((130, 300, 700))
    assert m.size == 1408 and int(m.sum()) == 1130
    assert m[:130].all() and not m[130:256].any() and m[256:556].all() and not m[556:640].any() and m[640:1340].all() and not m[1340:].any()
    assert ex.logical_mask((1280,)).all() and ex.logical_mask((1250,)).sum() == 1250 and ex.logical_mask((1250,)).size == 1280


@pytest.mark.parametrize("sizes,s", [((1280,), 40), ((1250,), 17), ((130, 300, 700), 16)])
def test_trmm_operands_are_exact_in_fp64(sizes, s):
    raw, L, Z, shift, ref = ex.trmm_operands(sizes, s, seed=1)
    mask = ex.logical_mask(sizes)
    pn, n = mask.size, int(mask.sum())
    assert raw.shape == (pn, pn) and L.shape == (n, n) and ref.shape == (n, s) and ref.dtype == np.int64
    assert np.array_equal(L, np.tril(L)) and L.min() == -8 and L.max() == 8 and Z.min() == -8 and Z.max() == 8
    # every partial sum is an integer below 2^17 (in ANY order: the bound is on the sum of the moduli)
    assert ex.trmm_partial_sum_bound(n) < 2 ** 17 < ex.EXACT_LIMIT
    assert int(np.max(np.abs(L) @ np.abs(Z) + np.abs(shift)[:, None])) <= ex.trmm_partial_sum_bound(n)
    # float64 in three orders of summation
    Lf, Zf, sf = L.astype(np.float64), Z.astype(np.float64), shift.astype(np.float64)
    assert np.array_equal(sf[:, None] + Lf @ Zf, ref)
    assert np.array_equal((Lf[:, ::-1] @ Zf[::-1]) + sf[:, None], ref)
    chunks = sum(Lf[:, c:c + 512] @ Zf[c:c + 512] for c in range(0, n, 512))
    assert np.array_equal(sf[:, None] + chunks, ref)
    # the storage: the operand below, garbage above, the identity in the padding
    up = np.triu(np.ones((pn, pn), dtype=bool), 1)
    assert np.all(np.isnan(raw[up]) | (raw[up] == 1e30)) and np.isnan(raw[up]).any() and (raw[up] == 1e30).any()
    low = np.where(up, 0.0, raw)
    assert np.all(np.isfinite(low)) and np.array_equal(low[np.ix_(mask, mask)], Lf)
    pad = ~mask
    if pad.any():
        assert np.array_equal(low[np.ix_(pad, pad)], np.eye(int(pad.sum()))) and not low[np.ix_(pad, mask)].any() and not low[np.ix_(mask, pad)].any()
    # the diagonal tiles hold garbage above their diagonals, and so does every tile above them
    assert not np.isfinite(raw[0, 1]) or raw[0, 1] == 1e30
    assert np.all(~np.isfinite(raw[:128, 128:256]) | (raw[:128, 128:256] == 1e30))


def test_the_public_path_sizes_stay_exact():
    """(n, s) = (2500, 130), the largest product of the GPU suite: partial sums up to 160 008, above 2^17 and far below 2^53."""
    assert 2 ** 17 < ex.trmm_partial_sum_bound(2500) == 160008 < ex.EXACT_LIMIT
    raw, L, Z, shift, ref = ex.trmm_operands((2500,), 3, seed=2)
    assert np.array_equal(shift[:, None].astype(np.float64) + L.astype(np.float64) @ Z.astype(np.float64), ref)


@pytest.mark.parametrize("sizes", [(200, 317), (130, 300, 700)])
def test_contraction_operands_are_exact_in_fp64(sizes):
    raw, r, v, q, t, diag = ex.contraction_operands(sizes, seed=3)
    mask = ex.logical_mask(sizes)
    pn, n = mask.size, int(mask.sum())
    assert ex.contraction_partial_sum_bound(n) < ex.EXACT_LIMIT
    keep = np.tril(np.ones((pn, pn), dtype=bool)) & mask[:, None] & mask[None, :]
    for name in ("ginv", "dG"):
        assert np.all(np.isfinite(raw[name][keep])) and np.abs(raw[name][keep]).max() == 4
        assert np.all(np.isnan(raw[name][~keep]) | (raw[name][~keep] == 1e30))
    A = np.where(keep, raw["ginv"], 0.0)[np.ix_(mask, mask)]
    B = np.where(keep, raw["dG"], 0.0)[np.ix_(mask, mask)]
    rf = r.astype(np.float64)
    # the kernel's own grouping in float64: per column j, w_j * sum_i f_ij w_i dG_ij; columns in two orders
    f = 2.0 * np.tril(np.ones((n, n)), -1) + np.eye(n)
    cols_q = rf * np.sum(f * rf[:, None] * B, axis=0)
    cols_t = np.sum(f * A * B, axis=0)
    for order in (slice(None), slice(None, None, -1)):
        assert float(np.sum(cols_q[order])) == float(q) and float(np.sum(cols_t[order])) == float(t)
    assert np.array_equal(np.diag(A), diag)
    assert abs(q) > 0 and abs(t) > 0                       # (a result of 0 would not see a dropped term)
