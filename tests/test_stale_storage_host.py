"""The layout predicates of tests/_stale_storage.py on NumPy arrays (no GPU): what of a matrix's padded storage the contract
defines, and that a deliberately dirty padding entry is found wherever it sits."""
import numpy as np
import pytest

import _stale_storage as S

BLOCKS = [129, 1, 128, 5]            # padded 256 | 128 | 128 | 128: tails of 127, 127, none and 123 rows
PN = 640


def clean(factored_rows):
    """A storage that keeps the contract: identity tails, garbage wherever nothing is defined."""
    rng = np.random.default_rng(1)
    raw = rng.standard_normal((PN, PN))
    raw[~S.defined_mask(PN, factored_rows)] = np.nan
    for poff, n, p in S.layout(BLOCKS):
        for r in range(poff + n, poff + p):
            raw[r, :r] = 0.0
            raw[r + 1:, r] = 0.0
            raw[r, r] = 1.0
    for t in range(factored_rows // 128):
        tile = raw[t * 128:(t + 1) * 128, t * 128:(t + 1) * 128]
        tile[np.triu_indices(128, 1)] = 0.0
    return raw


def test_layout_and_mask():
    assert S.layout(BLOCKS) == [(0, 129, 256), (256, 1, 128), (384, 128, 128), (512, 5, 128)]
    assert [S.padded(n) for n in (1, 127, 128, 129)] == [128, 128, 128, 256]
    m0, m1 = S.defined_mask(PN, 0), S.defined_mask(PN, 256)
    assert m0[200, 100] and m0[100, 100] and m0[129, 5] and not m0[5, 129] and not m0[100, 101] and not m0[130, 131]
    assert m0[300, 300] and not m0[300, 301] and not m0[0, 600]
    assert m1[100, 101] and m1[130, 131] and not m1[5, 129] and not m1[300, 301]          # factored diagonal tiles only
    assert int(m0.sum()) == 10 * 128 * 128 + 5 * (128 * 129 // 2)
    assert int(m1.sum()) - int(m0.sum()) == 2 * (128 * 127 // 2)


@pytest.mark.parametrize("factored_rows", [0, 256, 640])
def test_a_clean_storage_passes(factored_rows):
    assert S.contract_violations(clean(factored_rows), BLOCKS, factored_rows) == []


@pytest.mark.parametrize("value", [np.nan, 1e-300, -1.0, np.inf])
@pytest.mark.parametrize("where,what", [((130, 7), "padding row 130"), ((255, 254), "padding row 255"), ((200, 200), "on the diagonal"),
                                        ((639, 130), "padding"), ((400, 300), "padding column 300"), ((517, 0), "padding row 517"),
                                        ((636, 600), "padding")])
def test_a_dirty_padding_entry_is_found(where, what, value):
    raw = clean(0)
    raw[where] = value
    bad = S.contract_violations(raw, BLOCKS, 0)
    assert bad and any(what in b for b in bad), bad


def test_a_dirty_upper_triangle_of_a_factored_tile_is_found_and_of_an_unfactored_one_ignored():
    raw = clean(256)
    raw[300, 301] = 7.0                           # tile 2: not factored, nothing defined there
    assert S.contract_violations(raw, BLOCKS, 256) == []
    raw[130, 131] = 1e-300                        # tile 1: factored
    assert S.contract_violations(raw, BLOCKS, 256) == ["factored diagonal tile 1 is not zero above its diagonal"]


def test_same_bits_sees_payloads_and_signed_zeros():
    a = np.array([0.0, np.nan, 1.0])
    b = a.copy()
    assert S.same_bits(a, b)
    b[0] = -0.0
    assert not S.same_bits(a, b) and np.array_equal(a[[0, 2]], b[[0, 2]])
    c = a.copy()
    c.view(np.uint64)[1] ^= 1                     # another NaN
    assert np.isnan(c[1]) and not S.same_bits(a, c)
    assert not S.same_bits(a, a[:2])


def test_fills():
    assert S.FILLS == (0x00, 0xFF, 0x7F)
    nan, big = np.frombuffer(bytes([0xFF] * 8)), np.frombuffer(bytes([0x7F] * 8))
    assert np.isnan(nan[0]) and np.isfinite(big[0]) and big[0] > 1e306
