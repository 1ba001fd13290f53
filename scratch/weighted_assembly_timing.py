"""Timing of the weighted assembly (MEASUREMENTS.md, "Weighted assembly of variable-coefficient operators"): a 16 384 x 16 384
diagonal block, d = 2, product Matern-5/2; the generic assemble_kernel and the one-pair weighted kernel in alternation after a warm-up,
then 1, 4, 9 pairs and the nine pair descriptors on the generic kernel one by one.  HIP events through the profiling slots."""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # scratch/ sits in the repository root
sys.path[:0] = [ROOT, os.path.join(ROOT, "linpde-gp_amd")]
import numpy as np
import linpde_gp_amd as lp
from linpde_gp_amd import _engine
from linpde_gp_amd.linfuncops import diffops
from linpde_gp_amd.randprocs import _gaussian_process as gps

cf = lp.randprocs.covfuncs
ctx = _engine.default_context()
print(ctx.device_info())
n = 16384
X = np.random.default_rng(0).uniform(-1, 1, (n, 2))
P = _engine.Points(ctx, X)
k = cf.TensorProduct(cf.Matern((), nu=2.5, lengthscales=1.0), cf.Matern((), nu=2.5, lengthscales=0.7))
terms = [{(2, 0): -1.0, (0, 2): -1.0}, {(1, 0): 1.0}, {(0, 0): 2.0}]
W = np.random.default_rng(1).uniform(0.5, 1.5, (3, n))
M = _engine.GramMatrix(ctx, capacity_hint=n)
M.add_block(n)

def timed(label, fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    ctx.sync()
    out = []
    for _ in range(reps):
        ctx.profile_reset(); ctx.profile_enable(["assemble"])
        fn(); ctx.sync()
        p = ctx.profile_get()["assemble"]; ctx.profile_enable(False)
        out.append(p["ms"])
    out = np.array(out)
    print(f"{label}: median {np.median(out):.3f} ms  min {out.min():.3f}  max {out.max():.3f}  ({reps} runs, {p['launches']} launch, {p['bytes'] / 1e9:.2f} GB algorithmic)")
    return float(np.median(out))

lap = gps._lowered(k, terms[0], terms[0])
res = {}
# warm the clocks, then the generic kernel and the one-pair weighted kernel in alternation (same descriptor)
one = [(lap, 0, 0)]
ctx.set_option("asm_fast", 0)
for _ in range(60):
    M.assemble(lap, P, None, 0, 0)
ctx.sync()
ga, wa = [], []
for _ in range(12):
    for fn_, acc in ((lambda: M.assemble(lap, P, None, 0, 0), ga), (lambda: M.assemble_weighted(one, W[:1], None, P, None, 0, 0), wa)):
        ctx.profile_reset(); ctx.profile_enable(["assemble"]); fn_(); ctx.sync()
        acc.append(ctx.profile_get()["assemble"]["ms"]); ctx.profile_enable(False)
ga, wa = np.array(ga), np.array(wa)
print(f"ALTERNATING generic: median {np.median(ga):.3f} min {ga.min():.3f} max {ga.max():.3f} | weighted 1 pair: median {np.median(wa):.3f} min {wa.min():.3f} max {wa.max():.3f} | ratio of medians {np.median(wa) / np.median(ga):.3f}")
ctx.set_option("asm_fast", 0)
res["generic"] = timed("generic assemble_kernel, Lap k Lap (asm_fast = 0)", lambda: M.assemble(lap, P, None, 0, 0))
ctx.set_option("asm_fast", 1)
res["fast"] = timed("specialised assemble_fast_kernel, Lap k Lap", lambda: M.assemble(lap, P, None, 0, 0))
for A in (1, 2, 3):
    pairs = [(gps._lowered(k, terms[a], terms[b]), a, b) for a in range(A) for b in range(A)]
    res[A * A] = timed(f"weighted, {A * A} pair(s)", lambda: M.assemble_weighted(pairs, W[:A], None, P, None, 0, 0))
# the generic kernel on the identical 9-descriptor work: one launch per pair descriptor
tot = 0.0
ctx.set_option("asm_fast", 0)
for a in range(3):
    for b in range(3):
        d = gps._lowered(k, terms[a], terms[b])
        tot += timed(f"  generic, pair ({a},{b})", lambda: M.assemble(d, P, None, 0, 0), reps=5, warm=1)
ctx.set_option("asm_fast", 1)
print(f"sum of the 9 generic launches: {tot:.3f} ms; weighted 9 pairs: {res[9]:.3f} ms; ratio 1 pair / generic: {res[1] / res['generic']:.3f}")
