"""Throughput of the compact (Wendland) instantiations of the generic assembly and matrix-free kernels, and what skipping empty
tiles saves.  4096 x 16384, 2-D: a tensor product of two Wendland k = 2 factors (lengthscale 0.25 on [-1, 1]^2) on points sorted
along the first axis (tiles out of reach are skipped), on the same points shuffled (same entries, nothing skippable), and a
Matern-5/2 tensor product of the same shape (the specialised kernel, unchanged by the Wendland families).  Kernel time from the
library's profiling slots (`assemble`, `matvec`: events around the launches, no host copy inside), 3 warm-up calls, best and
median of 7.   usage: python scratch/wendland_rates.py [> profiles/wendland_rates.txt]"""
import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'linpde-gp_amd')
import numpy as np
import linpde_gp_amd as lp
from linpde_gp_amd import _engine

cf = lp.randprocs.covfuncs
ctx = _engine.default_context()
N0, N1, LS = 4096, 16384, 0.25
rng = np.random.default_rng(0)
X0, X1 = rng.uniform(-1, 1, (N0, 2)), rng.uniform(-1, 1, (N1, 2))
S0, S1 = X0[np.argsort(X0[:, 0])], X1[np.argsort(X1[:, 0])]
wend = cf.TensorProduct(cf.WendlandCovarianceFunction((), 2, LS), cf.WendlandCovarianceFunction((), 2, LS))
mat = cf.TensorProduct(cf.Matern((), nu=2.5, lengthscales=LS), cf.Matern((), nu=2.5, lengthscales=LS))
V = rng.standard_normal((N1, 4))
cases = [("Wendland k=2, sorted", wend, S0, S1), ("Wendland k=2, shuffled", wend, X0, X1), ("Matern-5/2 (specialised kernel)", mat, X0, X1)]


def tiles_out(A, B):
    """64 x 64 tiles whose bounding boxes are more than LS apart in some dimension (what the kernels skip)."""
    lo0, hi0 = [np.array([f(A[i:i + 64], axis=0) for i in range(0, len(A), 64)]) for f in (np.min, np.max)]
    lo1, hi1 = [np.array([f(B[i:i + 64], axis=0) for i in range(0, len(B), 64)]) for f in (np.min, np.max)]
    gap = np.maximum(np.maximum(lo0[:, None, :] - hi1[None, :, :], lo1[None, :, :] - hi0[:, None, :]), 0.0)
    return float((gap / LS > 1.0).any(axis=-1).mean())


def timed(slot, call):
    ms = []
    for rep in range(10):
        ctx.profile_reset(); ctx.profile_enable([slot])
        call()
        ctx.sync(); p = ctx.profile_get()[slot]; ctx.profile_enable(False)
        if rep >= 3:
            ms.append(p["ms"])
    return min(ms), float(np.median(ms)), p["launches"]


for name, k, A, B in cases:
    desc = k.lower()
    PA, PB = _engine.Points(ctx, A), _engine.Points(ctx, B)
    skip = tiles_out(A, B) if k is wend else 0.0
    best, med, n = timed("assemble", lambda: _engine.kernel_matrix(ctx, desc, PA, PB))
    gb = 8.0 * N0 * N1 / 1e9
    print(f"assemble {name}: {skip:.0%} of the tiles out of reach; {n} launch(es), best {best:.4f} ms, median {med:.4f} ms -> {gb / best * 1e3:.0f} GB/s of output", flush=True)
    best, med, n = timed("matvec", lambda: _engine.kernel_matvec(ctx, desc, PA, PB, V))
    print(f"matvec   {name}, 4 right-hand sides: {n} launch(es), best {best:.4f} ms, median {med:.4f} ms -> {N0 * N1 / best / 1e6:.1f} G entries/s", flush=True)
