"""The reference of tests/test_gpu_gemm_cyc_exact.py (tests/_cyc_reference.py) on the host: its set of written tiles is the one the
project's replay of the staircase enumeration returns (`lpgp_test_stair_enumerate`, tests/test_dist_cpu.py), for every launch of the
GPU test's table and every rank; and the table tells the right reference from three wrong ones.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _cyc_reference as cr
import _hooks

CAP = 4096
_out = (C.c_int32 * (2 * CAP))()


def _replay(pr, pc, r, c, nbt, T, row_lo, col_lo):
    n = _hooks.lib.lpgp_test_stair_enumerate(pr, pc, r, c, nbt, T, row_lo, col_lo, _out, CAP)
    assert 0 <= n <= CAP
    got = [tuple(x) for x in np.frombuffer(_out, dtype=np.int32, count=2 * n).reshape(n, 2)]
    assert len(got) == len(set(got))
    return set(got)


def _table():
    for pr, pc in cr.GRIDS:
        for nbt in cr.NBTS:
            for T in cr.TS:
                for case in cr.cases(nbt, T):
                    for r in range(pr):
                        for c in range(pc):
                            yield pr, pc, r, c, nbt, T, case


def test_table_covers_what_it_claims():
    rows = list(_table())
    assert len(rows) > 3000
    assert {(row[6].kt, row[4]) for row in rows} >= {(1, 1), (2, 2), (4, 4), (3, 4)}        # k of 1 and 4 tiles (and the ragged old panel)
    assert {row[6].tri for row in rows} == {1, 3} and {row[6].occ3 for row in rows} == {0, 1}
    assert {row[6].opts["gemm_band"] for row in rows} == {4, 8, 16}
    assert all(0 < case.g0 <= min(case.row_lo, case.col_lo) and case.col_lo < case.col_hi <= T for *_, T, case in rows)
    # some ranks own nothing of a region, some own no tile at all
    empty = [row for row in rows if not cr.plan(*row)]
    assert len(empty) > 100
    assert any(not cr.owned(pc, c, nbt, T) for pr, pc, r, c, nbt, T, case in rows)


def test_reference_tiles_are_the_replayed_enumeration():
    """Columns [col_lo, col_hi): the replay takes columns up to T only, so the set is the difference of two replays with the same rows."""
    for pr, pc, r, c, nbt, T, case in _table():
        want = _replay(pr, pc, r, c, nbt, T, case.row_lo, case.col_lo) - _replay(pr, pc, r, c, nbt, T, case.row_lo, case.col_hi)
        pl = cr.plan(pr, pc, r, c, nbt, T, case)
        assert cr.global_tiles(pr, pc, r, c, nbt, T, pl) == want, (pr, pc, r, c, nbt, T, case)
        # the operand rows: global tile minus the panel origin, inside the panel buffer
        rows, cols = cr.owned(pr, r, nbt, T), cr.owned(pc, c, nbt, T)
        for (lr, lc), (a, b) in pl.items():
            assert (a, b) == (rows[lr] - case.g0, cols[lc] - case.g0) and 0 <= b <= a < T - case.g0


@pytest.mark.parametrize("wrong", ["swap", "g0", "strict"])
def test_table_sees_a_wrong_reference(wrong):
    """my_r / my_c exchanged, the panel origin off by one tile, gr > gc instead of >=: each differs from the right plan on the table --
    and a differing plan is a differing matrix (integer operands: two tiles of P P^T, or a written and an unwritten tile, never agree)."""
    differing = [row for row in _table() if cr.plan(*row, wrong=wrong) != cr.plan(*row)]
    print(f"\n[cyc reference] {wrong}: {len(differing)} launches of the table differ")
    assert differing
    if wrong == "swap":       # only an asymmetric rank can show it: and every asymmetric grid does
        assert {row[:2] for row in differing} >= {(2, 1), (1, 2), (2, 2), (3, 2), (4, 1), (2, 4)}
    # in numbers, on the smallest differing launch
    pr, pc, r, c, nbt, T, case = min(differing, key=lambda row: (len(cr.owned(row[0], row[2], row[4], row[5])), row[5]))
    rng = np.random.default_rng(1)
    rows, cols = cr.owned(pr, r, nbt, T), cr.owned(pc, c, nbt, T)
    P = rng.integers(-1024, 1025, size=((T - case.g0 + 1) * cr.TILE, case.kt * cr.TILE)).astype(np.float64)   # (one spare tile row for "g0")
    C0 = rng.integers(-1024, 1025, size=(len(rows) * cr.TILE, len(cols) * cr.TILE)).astype(np.float64)
    PPt = P @ P.T
    good, bad = cr.plan(pr, pc, r, c, nbt, T, case), cr.plan(pr, pc, r, c, nbt, T, case, wrong=wrong)
    if wrong == "swap":       # (the exchanged rank has another storage shape: compare the written global tiles)
        assert cr.global_tiles(pr, pc, r, c, nbt, T, good) != cr.global_tiles(pr, pc, c, r, nbt, T, bad)
        return
    bad = {k: (a % (T - case.g0 + 1), b % (T - case.g0 + 1)) for k, (a, b) in bad.items()}       # ("g0": row -1 is some other row)
    assert not np.array_equal(cr.apply_plan(good, PPt, C0, *case.ab), cr.apply_plan(bad, PPt, C0, *case.ab))
