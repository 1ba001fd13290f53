"""High-precision reference of the greedy pivoted Cholesky of `csrc/pivchol.hip` (`lpgp_pivchol_*`) and the bounds the device is held
to (test_pivchol_reference.py on the CPU, test_gpu_pivchol.py on the device).  A plain module, not a conftest: NumPy, no device code.

The specification is the host loop of `randprocs/_matrix_free.PivotedCholeskyPreconditioner`.

* `one_step(L_prev, d, row)`: ONE step in `np.longdouble` from a given float64 state -- the pivot p = first argmax of d, the new row
  L[k] = (row - L[:k, p] @ L[:k]) / sqrt(d[p]) with the running d[p], the new diagonal max(d - L[k]^2, 0) with d[p] = 0.  `row` carries
  the noise entry already.  Checks against it are LOCAL: the state it starts from is the state of the code under test, so no
  conditioning-dependent amplification enters a bound.
* `replay(row_of, diag, pivots)`: the whole factorisation in `np.longdouble` from a given pivot list.
* `delta_of(d, d0, floor)`: max(mean(d), floor * d0) in longdouble.

Bounds (u = 2^-53; none is measured):
  row commit   |L[k, j] - ref| <= (k + 3) u (|g_j| + sum_t |L[t, p]| |L[t, j]|) / sqrt(d_p): k fma roundings, the square root, the
               division, and the noise add at j = p (the kernel has k + 2 roundings off the pivot column, k + 3 on it)
  diagonal     |d_new[j] - max(d[j] - L[k, j]^2, 0)| <= 2 u (d[j] + L[k, j]^2), against the L[k] the code itself produced
  sum of d     depth u sum|d|, depth = ceil(n / 65 536) + 16 (per-thread chain over trips of 256 workgroups x 256 threads, two
               256-wide trees), + 1 for the division by n
  small Gram   (ceil(n / 256) + 8 + 2) u |L| |L|^T: the per-thread fma chain, one 256-wide tree, and 2 for the shift on the diagonal
               (its rounding u (|L_a|^2 + delta) <= 2 u |L_a|^2 while delta <= L[a, p_a]^2, which the greedy rule gives)
each doubled where the second-order terms matter (stated at the use)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
ARGMAX_TRIP = 256 * 256       # rows one trip of the first argmax stage covers (256 workgroups of 256 threads)


def sum_depth(n):
    return -(-n // ARGMAX_TRIP) + 16


def gram_depth(n):
    return -(-n // 256) + 8 + 2


def one_step(L_prev, d, row):
    """(p, L_new, d_new) in longdouble from the float64 state (L_prev: k x n, d: n) and the evaluated row of the pivot."""
    L_prev = np.asarray(L_prev, dtype=np.double).reshape(-1, np.asarray(d).size)
    d = np.asarray(d, dtype=np.double)
    p = int(np.argmax(d))
    s = np.asarray(row).astype(LD) - L_prev[:, p].astype(LD) @ L_prev.astype(LD)
    L_new = s / np.sqrt(LD(d[p]))
    d_new = np.maximum(d.astype(LD) - L_new * L_new, LD(0))
    d_new[p] = 0
    return p, L_new, d_new


def commit_bound(L_prev, d, row, p):
    """(k + 3) u (|g| + sum_t |L[t, p]| |L[t]|) / sqrt(d_p), float64"""
    L_prev = np.asarray(L_prev, dtype=np.double).reshape(-1, np.asarray(d).size)
    k = L_prev.shape[0]
    return (k + 3) * U * (np.abs(np.asarray(row, dtype=np.double)) + np.abs(L_prev[:, p]) @ np.abs(L_prev)) / np.sqrt(d[p])


def diag_update(d, L_new, p):
    """(reference, bound) of the new diagonal given the row the code itself produced"""
    d, L_new = np.asarray(d, dtype=np.double), np.asarray(L_new, dtype=np.double)
    ref = np.maximum(d.astype(LD) - L_new.astype(LD) ** 2, LD(0))
    ref[p] = 0
    return ref, 2.0 * U * (d + L_new * L_new)


def replay(row_of, diag, pivots):
    """L (len(pivots) x n) and the remaining diagonal, longdouble, for the given pivots in their order.  `row_of(p)`: row p of G with
    its noise entry.  The diagonal is carried by the update rule, as the algorithm carries it."""
    d = np.asarray(diag).astype(LD).copy()
    n = d.size
    L = np.zeros((len(pivots), n), dtype=LD)
    for k, p in enumerate(pivots):
        s = np.asarray(row_of(p)).astype(LD) - L[:k, p] @ L[:k]
        L[k] = s / np.sqrt(d[p])
        d = np.maximum(d - L[k] * L[k], LD(0))
        d[p] = 0
    return L, d


def delta_of(d, d0, floor):
    d = np.asarray(d).astype(LD)
    return max(np.sum(d) / LD(d.size), LD(floor) * LD(d0))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the entries (0 / 0 counts as 0, anything / 0 as inf)"""
    err = np.abs(np.asarray(got).astype(LD) - np.asarray(ref).astype(LD)).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0
