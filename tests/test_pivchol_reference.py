"""tests/_pivchol_reference.py held against the class it restates, `PivotedCholeskyPreconditioner` on dense stand-ins
(`mr.build_preconditioner`), on the CPU.

* `one_step` from the class's own float64 state before every pivot: the same pivot, and the class's row within the commit bound
  (a BLAS dot of k terms, the subtraction, the square root, the division: k + 3 roundings at most).  The state before step k is
  rebuilt from the class's rows by its own update rule, statement by statement in float64, so it is the class's state bit for bit.
* `delta_of` on the final state against the class's delta (a float64 mean of n terms: n u of the mean of |d|).
* `replay` from the class's pivot list: every pivot row of G is reproduced by the factor, sum_{t <= k} L[t, p_k] L[t] = G[p_k], to the
  rounding of longdouble, 2 (k + 3) 2^-64 (|L|^T |L|)[p_k] -- the defining property of the algorithm, which needs no second
  implementation to compare with -- and the diagonal it carries matches diag(G - L^T L) at the same level or was clipped at 0."""
import numpy as np
import pytest

import _mfree_reference as mr
import _pivchol_reference as pv

LD, U = pv.LD, pv.U
CASES = [("matern52", 1, 1e-2, 200), ("matern52", 64, 1e-2, 200), ("expquad", 150, 1e-6, 17), ("matern52", 333, 1e-2, 200), ("expquad", 201, 1e-2, 0)]


@pytest.mark.parametrize("kernel,n,noise,rank", CASES)
def test_one_step_and_delta_against_the_class(kernel, n, noise, rank):
    c = mr.case(kernel, n, noise)
    pre, pivots = mr.build_preconditioner(c.G, rank)
    assert pre.rank == len(pivots) <= min(rank, n) and list(pre.pivots) == pivots
    d = np.diag(c.G).copy()
    d0 = float(np.max(d))
    worst = 0.0
    for k, p in enumerate(pivots):
        p_ref, L_ref, d_ref = pv.one_step(pre.L[:k], d, c.G[p])
        assert p_ref == p and d[p] > mr.PIVOT_RTOL * d0
        worst = max(worst, pv.worst_ratio(pre.L[k], L_ref, pv.commit_bound(pre.L[:k], d, c.G[p], p)))
        d_before = d
        d = np.maximum(d_before - pre.L[k] * pre.L[k], 0.0)       # the class's own update, in float64
        d[p] = 0.0
        ref, bound = pv.diag_update(d_before, pre.L[k], p)
        assert pv.worst_ratio(d, ref, bound) <= 1.0 and d[p] == 0.0
    if pre.rank < min(rank, n):
        assert np.max(d) <= mr.PIVOT_RTOL * d0                 # the rtol stop is why the class stopped
    delta = pv.delta_of(d, d0, mr.DELTA_FLOOR)
    err = abs(LD(pre.delta) - delta)
    print(f"{c} rank {rank}: {pre.rank} pivots, worst row error / bound {worst:.3f}, delta error {float(err):.2e}")
    assert worst <= 1.0
    assert err <= n * U * float(np.mean(np.abs(d))) + U * float(delta)


@pytest.mark.parametrize("kernel,n,noise,rank", CASES[1:4])
def test_replay_reproduces_the_pivot_rows(kernel, n, noise, rank):
    c = mr.case(kernel, n, noise)
    pre, pivots = mr.build_preconditioner(c.G, rank)
    L, d = pv.replay(lambda p: c.G[p], np.diag(c.G), pivots)
    assert L.shape == (len(pivots), n) and d.shape == (n,)
    absLL = np.abs(L).T @ np.abs(L)
    got = L.T @ L
    eps = 2.0 ** -64
    worst = 0.0
    for k, p in enumerate(pivots):
        # rows t > k are zero in column p_k (their d[p_k] was 0 ... to rounding: they are what the clipping left)
        worst = max(worst, pv.worst_ratio(L[: k + 1, p] @ L[: k + 1], c.G[p], 2.0 * (k + 3) * eps * absLL[p].astype(np.double)))
        assert d[p] == 0
    resid = np.diag(c.G).astype(LD) - np.diag(got)
    clipped = d == 0
    ok = np.abs(d - resid) <= 2.0 * (len(pivots) + 3) * eps * np.diag(absLL)
    print(f"{c} rank {rank}: pivot rows reproduced, worst error / bound {worst:.3f}; {int(np.sum(clipped))} diagonal entries at 0")
    assert worst <= 1.0
    assert np.all(ok | clipped) and np.all(d >= 0)
