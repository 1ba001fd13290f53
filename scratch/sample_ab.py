"""A/B probe of `u.sample`: the device route (`lpgp_mat_sub_inner`, `lpgp_potrf`, `lpgp_mat_factor_matmul`) against the only
route there was before it, `C = np.linalg.cholesky(u.cov.matrix(x) + delta I); mean + z @ C.T` in NumPy, around the SAME
posterior -- cold (first sample at the points) and warm (kept factor) -- at c3 (16 896 observations, M = 4 096, 16 draws) and
at c1 (the reference's 1-D Poisson size).  Three repetitions after a warm-up, median and range, device synchronised.  Then
the product kernel alone (HIP events, profiling slot "trmm") at n = 4 096 and 16 384, s = 16, against its read bound 4 n^2
bytes at 6.3 TB/s, and whether the default damping factors the c3 posterior (noise-free PDE block) and the smallest power of
ten that does.

    python scratch/sample_ab.py [--skip-host] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "linpde-gp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import linpde_gp_amd as lp                      # noqa: E402
from linpde_gp_amd import _engine, problems     # noqa: E402


def timed(fn, ctx, reps=3):
    fn()                                        # warm-up
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def ab(name, wl, damping, draws, skip_host):
    ctx = _engine.default_context()
    u, _, _ = problems.condition_and_predict(wl)
    x = wl.Xtest
    M = x.shape[0]
    scan = damping_scan(u, x)
    works = [10.0 ** int(k[2:]) for k, ok in scan.items() if ok]
    if not scan.get("1e-6", False):
        damping = 10.0 * min(works)             # the default does not factor here: one decade above the smallest that does
    delta = damping * u._prior_diag()
    z = np.random.default_rng(0).standard_normal((draws, M))

    class Fixed:
        def standard_normal(self, shape):
            return z.reshape(shape)

    def device_cold():
        u._sample_cache = None
        return u.sample(Fixed(), x, size=draws, damping=damping)

    def device_warm():
        return u.sample(Fixed(), x, size=draws, damping=damping)

    def host():
        C = np.linalg.cholesky(u.cov.matrix(x) + delta * np.eye(M))
        return u.mean(x) + z @ C.T

    out = {"workload": name, "n_obs": wl.n_total, "M": M, "draws": draws, "damping": damping, "damping_factors": scan}
    out["device_cold"] = timed(device_cold, ctx)
    out["device_warm"] = timed(device_warm, ctx)
    if not skip_host:
        out["host"] = timed(host, ctx)
        out["host_over_device_cold"] = out["host"]["median_ms"] / out["device_cold"]["median_ms"]
        d, h = device_warm(), host()
        out["max_abs_difference"] = float(np.max(np.abs(d - h)))
    return out, u


def product_rate(n, s=16):
    ctx = _engine.default_context()
    rng = np.random.default_rng(1)
    mat = _engine.GramMatrix(ctx, n)
    mat.add_block(n)
    x = np.sort(rng.uniform(-1, 1, (n, 1)), axis=0)
    mat.assemble(lp.randprocs.covfuncs.Matern((1,), nu=2.5, lengthscales=0.3).lower(), _engine.Points(ctx, x), None, 0, 0)
    mat.add_diag(0, None, 1.0)
    assert mat.potrf() == 0
    Z = rng.standard_normal((n, s))
    mat.factor_matmul(Z)
    ctx.profile_enable(["trmm"])
    ms = []
    try:
        for _ in range(5):
            ctx.profile_reset()
            mat.factor_matmul(Z)
            ms.append(ctx.profile_get()["trmm"]["ms"])
    finally:
        ctx.profile_enable(False)
    bound_ms = 4.0 * n * n / 6.3e12 * 1e3
    return {"n": n, "s": s, "kernel_ms_median": float(np.median(ms)), "kernel_ms_min": float(min(ms)), "kernel_ms_max": float(max(ms)),
            "read_bound_ms": bound_ms, "fraction_of_read_bound": bound_ms / float(np.median(ms))}


def damping_scan(u, x):
    res = {}
    for e in range(-12, -2):
        u._sample_cache = None
        try:
            u.sample(np.random.default_rng(0), x, damping=10.0 ** e)
            res[f"1e{e}"] = True
        except np.linalg.LinAlgError:
            res[f"1e{e}"] = False
    u._sample_cache = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    report = {}
    r, _ = ab("c1 poisson1d 512 + 32", problems.poisson_1d(512, n_bdry_repeats=16, noise_var=1e-4, m=256), 1e-6, 16, args.skip_host)
    report["c1"] = r
    print(json.dumps(r), flush=True)
    wl = problems.poisson_2d(n_side=128, n_bdry=128, m_side=64)
    r, u = ab("c3 poisson2d 128 x 128", wl, 1e-6, 16, args.skip_host)
    report["c3"] = r
    print(json.dumps(r), flush=True)
    del u
    report["product"] = [product_rate(4096), product_rate(16384)]
    print(json.dumps(report["product"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
