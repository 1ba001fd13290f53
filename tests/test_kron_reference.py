"""The high-precision grid-block reference of tests/_kron_reference.py, checked on the CPU before the device is held against it
(tests/test_gpu_kron_exact.py):

* it agrees with the existing oracle `oracle.covfuncs.LkL` on the flattened mesh, entry by entry and relative to the envelope; the
  oracle's own worst ratio `rho_oracle = max |LkL - G| / E` per case is what the device bound K is derived from (MEASUREMENTS.md,
  "Entry-exact Kronecker assembly"): K = 4 * max rho_oracle;
* every case SEES a transposed factor: the reference with one factor transposed misses the bound, so an expansion that transposes,
  or on these non-equispaced and unequal grids shifts or swaps a factor, cannot pass;
* the case ids cover every kernel `launch_assemble_kron` can pick on one GPU.
"""
import numpy as np
import pytest

from oracle import covfuncs as ocf

import _kron_reference as kr
from test_gpu_kron_exact import K

CASES = kr.CASES


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_reference_matches_the_oracle_and_sees_a_transposed_factor(case):
    G, E = case.reference()
    assert np.all(np.isfinite(G.astype(np.double))) and np.all(E >= 0)
    X0, X1 = case.mesh()
    rho, pos = kr.worst_ratio(ocf.LkL(case.kernel, case.L0, case.L1, X0, X1), G, E)
    print(f"rho_oracle {case.id}: {rho / kr.EPS:.2f} eps at {case.describe(pos)}")
    # the oracle is float64: a wrong formula in the reference would be off by O(1), not by a few eps
    assert rho <= K, (case.id, rho, case.describe(pos))
    # |G| <= E by construction
    assert np.all(np.abs(G) <= E * (1 + 1e-15))
    d = case.flip_dim()
    Gt, _ = case.reference(flip_dim=d)
    seen, pos = kr.worst_ratio(Gt.astype(np.double), G, E, case.mask())
    assert seen > 1e6 * K, f"{case.id}: transposing factor {d} moves no checked entry by more than {seen:.2e} E"


def test_the_cases_cover_every_single_gpu_kernel_of_the_dispatcher():
    ids = {(c.kernel_name, c.kind) for c in CASES}
    want = ["kron2w<4>", "kron2<4>", "kron2<8>"] + [f"kron_expand<{D},{nu}>" for D, nus in ((2, (2, 4, 8, 16)), (3, (2, 4, 8, 16)),
                                                                                           (4, (2, 4, 8, 16))) for nu in nus]
    for name in want:
        for kind in ("off", "diag"):
            assert (name, kind) in ids, (name, kind)
    assert len({c.id for c in CASES}) == len(CASES)
    # rows and columns differ in every extent (an extent of 1 on both sides aside), so no two factors are exchangeable
    for c in CASES:
        if c.kind == "off":
            assert all(r != s or r == 1 for r, s in zip(c.rows, c.cols)), c.id
        # an odd total order in the dimension whose transposition the case has to see
        d = c.flip_dim()
        assert any((a[d] + b[d]) % 2 for a in c.L0 for b in c.L1), c.id


def test_one_dimensional_factor_against_direct_differentiation():
    """The polynomial-times-exponential form against SymPy's derivative of the kernel evaluated directly (no reduction), 40 digits."""
    import mpmath
    import sympy as sp
    x, y = sp.symbols("x y", real=True)
    x0, x1 = np.array([0.3, 0.9, 1.4]), np.array([0.1, 0.9, 1.2, 1.45])
    for factor, expr in ((("matern", 2.5, 0.9), None), (("expquad", 0.8), sp.exp(-(x - y) ** 2 / (2 * sp.Rational(0.8) ** 2)))):
        for n0, n1 in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (2, 2)):
            M, E = kr.factor_matrices(factor, [(n0, n1)], x0, x1)[(n0, n1)]
            for i, u in enumerate(x0):
                for j, v in enumerate(x1):
                    if expr is None:
                        if u == v:
                            continue
                        s = sp.sqrt(5) / sp.Rational(0.9) * (x - y) * (1 if u > v else -1)
                        e = (1 + s + s ** 2 / 3) * sp.exp(-s)
                    else:
                        e = expr
                    with mpmath.workdps(40):
                        ref = sp.diff(e, *([x] * n0), *([y] * n1)) if n0 + n1 else e
                        ref = float(sp.N(ref.subs({x: sp.Rational(float(u)), y: sp.Rational(float(v))}), 40))
                    assert abs(float(M[i, j]) - ref) <= 4e-16 * float(E[i, j]), (factor, n0, n1, i, j)
