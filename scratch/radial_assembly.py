"""Rate of the radial Matern assembly (second-order operators on an isotropic Matern prior) against the first-order isotropic block:
a 16 384^2 diagonal block (lower triangle) on scattered points, d = 2, nu = 5/2.  With LPGP_ASM_DIAG=1 (stores only) / =2
(evaluation only) in the environment the same launches tell whether the kernel is bound by its evaluation or by its stores."""
import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'linpde-gp_amd')
import numpy as np
import linpde_gp_amd as lp
from linpde_gp_amd import _engine
cf = lp.randprocs.covfuncs
ctx = _engine.default_context()
n = 16384
X = np.random.default_rng(0).uniform(-1, 1, (n, 2))
P = _engine.Points(ctx, X)
k = cf.Matern((2,), nu=2.5, lengthscales=[0.3, 0.25])
mlap = {(2, 0): -1.0, (0, 2): -1.0}
v = {(1, 0): 0.7, (0, 1): -0.4}
lp.config.isotropic_matern_higher_order = True
cases = [("first-order isotropic (<v, grad>, <v, grad>), family 3", cf.lower_groups(k._base_groups(), v, v)),
         ("radial (-Lap, -Lap), family 4", cf.lower_groups(k._base_groups(), mlap, mlap)),
         ("radial (id, -Lap), family 4", cf.lower_groups(k._base_groups(), {(0, 0): 1.0}, mlap))]
for name, desc in cases:
    M = _engine.GramMatrix(ctx, capacity_hint=n)
    M.add_block(n)
    best = 1e9
    for rep in range(5):
        ctx.profile_reset(); ctx.profile_enable(["assemble"])
        M.assemble(desc, P, None, 0, 0)
        ctx.sync(); p = ctx.profile_get()["assemble"]; ctx.profile_enable(False)
        best = min(best, p["ms"])
    print(f"{name}: {p['bytes'] / p['launches'] / 1e9:.3f} GB per launch, best {best:.4f} ms -> {p['bytes'] / p['launches'] / best / 1e9:.3f} TB/s", flush=True)
    del M
