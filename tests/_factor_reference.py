"""Long-double references computed from a GIVEN lower-triangular factor L (float64 in, `np.longdouble` inside), for the suite
that holds csrc/evidence.hip and the forward half of the single-vector solve to the device's own factor
(test_gpu_evidence_backward.py): with L shared between the device and the reference the cond-bound error of the factorisation
drops out and a measure sees the solve, the column sums, the reductions and the epilogue alone; lower_tmv() and backward_error_t()
are the transposed forms for the backward substitutions (test_gpu_solve_t_backward.py).  Checked against 50-digit
mpmath in test_factor_reference.py.  A plain module the suites import, not a conftest."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
HALF_LOG_2PI = LD(0.5) * np.log(LD(8) * np.arctan(LD(1)))      # 1/2 log 2 pi in long double


def forward(L, r):
    """z = L^{-1} r by rows: z_i = (r_i - sum_{j < i} L_ij z_j) / L_ii."""
    n = L.shape[0]
    z = np.zeros(n, dtype=LD)
    rl = np.asarray(r).astype(LD)
    for i in range(n):
        z[i] = (rl[i] - L[i, :i].astype(LD) @ z[:i]) / LD(L[i, i])
    return z


def inverse(L):
    """W = L^{-1} by rows (lower triangular): W[i, :i + 1] = (e_i - L[i, :i] W[:i, :i + 1]) / L_ii."""
    n = L.shape[0]
    W = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(L[i, :i].astype(LD) @ W[:i, :i + 1])
        row[i] += LD(1)
        W[i, :i + 1] = row / LD(L[i, i])
    return W


def inverse_diag(W):
    """d_j = sum_i W_ij^2 = diag((L L^T)^{-1})_j for W = L^{-1}."""
    return np.sum(W * W, axis=0)


def logdet(diag):
    """2 sum log L_ii and 2 sum |log L_ii| (the scale an absolute bound on the sum's error is stated against)."""
    lg = np.log(np.asarray(diag).astype(LD))
    return LD(2) * np.sum(lg), LD(2) * np.sum(np.abs(lg))


def loo(w, d, y):
    """The leave-one-out formulas (GPML eqs. 5.10 - 5.12) from w = G^{-1} r, d = diag(G^{-1}) and the observations y:
    mean = y - w / d, var = 1 / d, logp = 1/2 log d - 1/2 w^2 / d - 1/2 log 2 pi."""
    w, d, y = (np.asarray(a).astype(LD) for a in (w, d, y))
    return y - w / d, LD(1) / d, LD(0.5) * np.log(d) - LD(0.5) * w * w / d - HALF_LOG_2PI


def lower_mv(L, x, absolute=False):
    """L x (absolute: |L| |x|) in long double, by rows left of the diagonal."""
    xl = np.asarray(x).astype(LD)
    if absolute:
        xl = np.abs(xl)
    out = np.empty(L.shape[0], dtype=LD)
    for i in range(0, L.shape[0], 512):
        e = min(i + 512, L.shape[0])
        blk = L[i:e, :e].astype(LD)
        out[i:e] = (np.abs(blk) if absolute else blk) @ xl[:e]
    return out


def backward_error(L, z, r):
    """Componentwise backward error of L z = r: max_i |r - L z|_i / (|L| |z| + |r|)_i with the residual in long double; 0/0
    counts 0, a nonzero residual over 0 fails (the convention of test_gpu_predict_backward.py)."""
    rl = np.asarray(r).astype(LD)
    res = np.abs(rl - lower_mv(L, z))
    den = lower_mv(L, z, absolute=True) + np.abs(rl)
    zero = den == 0
    assert not np.any(res[zero] != 0), "a nonzero residual where |L||z| + |r| is zero"
    return float(np.max(np.where(zero, LD(0), res / np.where(zero, LD(1), den))))


def relative_error(got, ref):
    """max_i |got_i - ref_i| / |ref_i| (a zero reference entry must be met exactly)."""
    ref = np.asarray(ref).astype(LD)
    err = np.abs(np.asarray(got).astype(LD) - ref)
    zero = ref == 0
    assert not np.any(err[zero] != 0), "a nonzero value where the reference is exactly zero"
    return float(np.max(np.where(zero, LD(0), err / np.where(zero, LD(1), np.abs(ref)))))


def lower_tmv(L, x, absolute=False):
    """L^T x (absolute: |L|^T |x|) in long double for a vector or the columns of a matrix x, by row slabs of L: only the columns
    left of a slab's end take part."""
    xl = np.asarray(x).astype(LD)
    if absolute:
        xl = np.abs(xl)
    out = np.zeros(xl.shape, dtype=LD)
    for i in range(0, L.shape[0], 512):
        e = min(i + 512, L.shape[0])
        blk = L[i:e, :e].astype(LD)
        out[:e] += (np.abs(blk) if absolute else blk).T @ xl[i:e]
    return out


def backward_error_t(L, x, y):
    """Componentwise backward error of L^T x = y: max_i |y - L^T x|_i / (|L^T| |x| + |y|)_i with the residual in long double, the
    conventions of backward_error(); for matrices x, y the maximum is taken per column and an array comes back."""
    yl = np.asarray(y).astype(LD)
    res = np.abs(yl - lower_tmv(L, x))
    den = lower_tmv(L, x, absolute=True) + np.abs(yl)
    zero = den == 0
    assert not np.any(res[zero] != 0), "a nonzero residual where |L^T||x| + |y| is zero"
    e = np.max(np.where(zero, LD(0), res / np.where(zero, LD(1), den)), axis=0)
    return float(e) if e.ndim == 0 else e.astype(np.float64)


# ---- the two-stage reductions of csrc/evidence.hip: their launch shape and the roundings on a path ---------------------------------
EV_THREADS = 256          # threads of a workgroup of evidence_partial_kernel / loo_epilogue_kernel
EV_MAX_WGS = 256          # workgroups at most: the final kernel adds one partial per thread


def reduction_workgroups(pn, max_wgs=0):
    """Workgroups of stage 1 over `pn` padded rows: one per 256 rows, at most 256; `max_wgs` > 0 (the test hooks' cap) at most that."""
    nwg = min(-(-pn // EV_THREADS), EV_MAX_WGS)
    return min(nwg, max_wgs) if max_wgs > 0 else nwg


def reduction_depth(pn, max_wgs=0):
    """k: the rows a thread of stage 1 adds at most -- row i goes to thread i mod (256 nwg), so k = ceil(pn / (256 nwg))."""
    return -(-pn // (EV_THREADS * reduction_workgroups(pn, max_wgs)))


def sum_roundings(k):
    """Roundings on the longest path from a term to the result of a two-stage reduction whose threads add k terms each: k in the
    thread (one fma or add per term, the first onto 0.0), then 6 shuffle adds and 2 adds over the four waves in stage 1, the partial
    read as it is, 6 shuffle adds and 2 adds over the waves in stage 2: 16 + k."""
    return 16 + k


def sum_ulps(k):
    """Bound of a sum of terms of one sign, in u x the sum: (1 + u)^m - 1 with m = sum_roundings(k) is below (m + 3) u for every m a
    launch can have (m u << 1); the margin of 3 is the one the bound has carried at k = 1, where it reads 20."""
    return float(sum_roundings(k) + 3)


def log_ulps(k, base=7.0):
    """Bound of the log det term in u 2 sum |log L_ii|: `base` covers the reduction at k = 1 (where the per-thread add 0 + log is exact)
    and the device log's own error; each of the k - 1 further adds of a thread rounds once, at most u x the sum of the moduli."""
    return float(base + (k - 1))


def two_stage_sum(terms, nwg):
    """The sum of `terms` (float64) in the order of evidence_partial_kernel + evidence_final_kernel with `nwg` workgroups, in float64:
    thread t of workgroup b adds the terms b 256 + t, + nwg 256, ... in order; lanes by shuffles (offset 32, 16, ..., 1), the four
    waves as (0 + 1) + (2 + 3); stage 2 the same over the partials, one per thread.  A host model to hold the bound to."""
    terms = np.asarray(terms, dtype=np.float64)

    def block_sum(v):                             # v: 256 values, one per thread
        v = v.reshape(4, 64).copy()
        for off in (32, 16, 8, 4, 2, 1):
            shifted = np.zeros_like(v)
            shifted[:, :64 - off] = v[:, off:]
            shifted[:, 64 - off:] = v[:, 64 - off:]       # (a lane beyond the wave reads its own value; lane 0 never depends on it)
            v = v + shifted
        return (v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0])

    assert 1 <= nwg <= EV_MAX_WGS
    part = np.zeros(EV_THREADS)
    for b in range(nwg):
        acc = np.zeros(EV_THREADS)
        for i0 in range(b * EV_THREADS, terms.size, nwg * EV_THREADS):
            chunk = terms[i0:i0 + EV_THREADS]
            acc[:chunk.size] = acc[:chunk.size] + chunk
        part[b] = block_sum(acc)
    return block_sum(part)
