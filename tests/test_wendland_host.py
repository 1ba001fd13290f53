"""Wendland compact-support priors (`LPGP_WENDLAND`, `LPGP_WENDLAND_ISO`), the part that needs no GPU: the polynomials against
the literature, the Python lowering and its refusals, the NumPy helper against the exact blocks (`_wendland_reference.py`), the
C++ lowering + the shared evaluation core on the host under AddressSanitizer / UBSan (`csrc/hosttest/wendland_check.cpp`, a
stand-alone program run as a subprocess), and the posterior problem of the GPU test in fp64 LAPACK against a refined solve."""
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "linpde-gp_amd", "csrc")
sys.path.insert(0, HERE)
import _wendland_reference as ref  # noqa: E402

EPS = 2.0**-53
N0, N1 = 40, 24                      # block size of the CPU checks (the device tests use 150 x 70)

# (d, k): exponent of (1 - r) and the polynomial up to a constant factor (Wendland 2004, Table 9.1, and the d = 5 column)
LITERATURE = {
    (1, 0): (1, [1]), (1, 1): (3, [1, 3]), (1, 2): (5, [1, 5, 8]),
    (3, 0): (2, [1]), (3, 1): (4, [1, 4]), (3, 2): (6, [3, 18, 35]), (3, 3): (8, [1, 8, 25, 32]),
    (5, 0): (3, [1]), (5, 1): (5, [1, 5]), (5, 2): (7, [1, 7, 16]),
}


@pytest.mark.parametrize("d,k", sorted(LITERATURE))
def test_polynomials_against_the_literature(d, k):
    e, q = ref.factored(d, k)
    want_e, want_q = LITERATURE[(d, k)]
    assert e == want_e
    assert [c / q[0] for c in q] == [Fraction(c, want_q[0]) for c in want_q]
    assert ref.phi(d, k)[0] == 1 and sum(ref.phi(d, k)) == 0        # phi(0) = 1, phi(1) = 0
    # the odd coefficients below 2 k + 1 vanish: what makes phi'/s and (phi'' - phi'/s)/s^2 polynomials
    assert all(c == 0 for c in ref.phi(d, k)[1:2 * k + 1:2])


def test_expanded_coefficients_are_large_and_the_factored_ones_positive():
    """The figures of the design decision: sum |coefficients| of phi expanded in r, and q_0 > 0."""
    sums = {(d, k): round(sum(abs(c) for c in ref.phi(d, k))) for d, k in ((1, 3), (3, 3), (4, 3))}
    print(sums)
    assert sums == {(1, 3): 1110, (3, 3): 3718, (4, 3): 11669}
    for d in (1, 2, 3, 4):
        for k in range(4):
            assert all(c > 0 for c in ref.factored(d, k)[1])


def test_python_lowering_and_refusals():
    import linpde_gp_amd as lp
    from linpde_gp_amd import _lib
    from linpde_gp_amd.linfuncops import diffops
    cf = lp.randprocs.covfuncs
    assert (_lib.WENDLAND, _lib.WENDLAND_ISO) == (5, 6)
    k1 = cf.WendlandCovarianceFunction((), k=2, lengthscales=0.7)
    assert (k1.d, k1.k, float(k1.lengthscales)) == (1, 2, 0.7)
    (g,) = k1.lower()
    assert g["family"] == [5] and g["p"] == [2] and g["lengthscale"] == [0.7]
    assert cf.WendlandCovarianceFunction((1,), k=1).lower()[0]["family"] == [5]
    k3 = cf.WendlandCovarianceFunction((3,), k=2, lengthscales=[0.5, 1.0, 2.0])
    assert (k3.d, k3.k) == (3, 2) and list(k3.lengthscales) == [0.5, 1.0, 2.0]
    (g,) = k3.lower()
    assert g["family"] == [6] * 3 and g["p"] == [2] * 3 and g["lengthscale"] == [0.5, 1.0, 2.0]
    arr = _lib.make_kdesc_array(k3.lower())
    assert list(arr[0].family[:3]) == [6, 6, 6] and list(arr[0].p[:3]) == [2, 2, 2]
    assert list(_lib.make_kdesc_array(k1.lower())[0].family[:1]) == [5]
    assert float(cf.WendlandCovarianceFunction((2,), k=1).lengthscales) == 1.0          # the reference's default
    # a TensorProduct factor, beside a Matern factor
    tp = cf.TensorProduct(cf.WendlandCovarianceFunction((), k=2, lengthscales=0.7), cf.Matern((), nu=2.5, lengthscales=0.6))
    (g,) = (-1.0 * diffops.Laplacian((2,)))(tp, argnum=0).lower()
    assert g["family"] == [5, 1] and g["p"] == [2, 2]
    assert sorted((c, tuple(a), tuple(b)) for c, a, b in g["terms"]) == [(-1.0, (0, 2), (0, 0)), (-1.0, (2, 0), (0, 0))]
    # sums keep one group per summand
    assert [gg["family"] for gg in (k3 + cf.Matern((3,), nu=1.5)).lower()] == [[6] * 3, [3] * 3]
    # refusals
    for bad in (-1, 4, 1.5):
        with pytest.raises(NotImplementedError, match="k = 0, 1, 2, 3"):
            cf.WendlandCovarianceFunction((2,), k=bad)
    with pytest.raises(NotImplementedError):
        cf.WendlandCovarianceFunction((5,), k=1)
    with pytest.raises(ValueError, match="positive"):
        cf.WendlandCovarianceFunction((2,), k=1, lengthscales=[1.0, 0.0])
    with pytest.raises(ValueError, match="at most 2k"):
        cf.lower_groups(k1._base_groups(), {(3,): 1.0}, {(2,): 1.0})
    cf.lower_groups(k1._base_groups(), {(2,): 1.0}, {(2,): 1.0})
    with pytest.raises(ValueError, match="at most 2k"):
        diffops.Laplacian((2,))(cf.TensorProduct(cf.WendlandCovarianceFunction((), k=0), cf.WendlandCovarianceFunction((), k=2)), argnum=0).lower()
    D = diffops.DirectionalDerivative([1.0, -2.0, 0.5])
    with pytest.raises(NotImplementedError, match="TensorProduct"):
        diffops.Laplacian((3,))(k3, argnum=0).lower()
    with pytest.raises(ValueError, match="k = 0"):
        D(cf.WendlandCovarianceFunction((3,), k=0), argnum=1).lower()
    with pytest.raises(NotImplementedError, match="TensorProduct"):
        D(D(cf.WendlandCovarianceFunction((3,), k=1), argnum=1), argnum=0).lower()
    D(cf.WendlandCovarianceFunction((3,), k=1), argnum=1).lower()
    D(D(k3, argnum=1), argnum=0).lower()
    # the C lowering refuses what the Python layer would not send
    with pytest.raises(_lib.LpgpError, match="lengthscale"):
        v = _lib.C.c_double()
        grp = dict(k1.lower()[0], dlog_lengthscale=1)
        _lib.check(_lib.lib.lpgp_kernel_diag(None, _lib.make_kdesc_array([grp]), 1, _lib.C.byref(v)), "kernel_diag")


def _points(name, d, n0=N0, n1=N1):
    rng = np.random.default_rng(sum(map(ord, name)))
    return ref.dyadic_points(rng, n0, d), ref.dyadic_points(rng, n1, d)


@pytest.fixture(scope="module")
def exact_blocks():
    """name -> (kernel, L0, L1, X0, X1, G, E, OUT): every derivative case once, plus plain kernels on random (non-dyadic) points."""
    out = {}
    for name, kern, L0, L1 in ref.derivative_cases():
        d = len(next(iter(L0)))
        X0, X1 = _points(name, d)
        out[name] = (kern, L0, L1, X0, X1, *ref.exact_block(kern, L0, L1, X0, X1))
    rng = np.random.default_rng(5)
    for d, k in ((1, 0), (1, 3), (2, 1), (3, 2), (4, 3)):
        X0, X1 = rng.uniform(-1, 1, (N0, d)), rng.uniform(-1, 1, (N1, d))
        kern = [(1.0, ("prod", [("w", k, 0.7)]))] if d == 1 else [(1.0, ("iso", k, [0.9, 0.7, 1.1, 1.3][:d]))]
        out[f"plain_d{d}_k{k}"] = (kern, ref.identity(d), ref.identity(d), X0, X1, *ref.exact_block(kern, ref.identity(d), ref.identity(d), X0, X1))
    # sorted point sets: 16-point runs far out of each other's reach, entries with r == 1 exactly (what the tile decision is about)
    X0, X1 = np.arange(N0)[:, None] / 16.0, 0.5 + np.arange(N1)[:, None] / 16.0
    kern = [(1.0, ("prod", [("w", 2, 0.5)]))]
    out["sorted_1d"] = (kern, {(1,): 1.0}, {(1,): 1.0}, X0, X1, *ref.exact_block(kern, {(1,): 1.0}, {(1,): 1.0}, X0, X1))
    X0 = np.column_stack([np.sort(rng.uniform(-1, 1, N0)), rng.uniform(-1, 1, N0)])
    X1 = np.column_stack([np.sort(rng.uniform(-1, 1, N1)), rng.uniform(-1, 1, N1)])
    kern = [(1.0, ("iso", 2, [0.3, 0.4]))]
    out["sorted_iso"] = (kern, ref.identity(2), ref.identity(2), X0, X1, *ref.exact_block(kern, ref.identity(2), ref.identity(2), X0, X1))
    return out


def test_numpy_helper_vs_exact(exact_blocks):
    """|helper - exact| <= HELPER_BOUND eps E for every entry, exactly 0 outside the support; prints the worst ratio (the figure
    K_DEVICE = 4 x is derived from)."""
    worst = 0.0
    for name, (kern, L0, L1, X0, X1, G, E, OUT) in exact_blocks.items():
        H = ref.helper_block(kern, L0, L1, X0, X1)
        assert np.isfinite(H).all() and (H[OUT] == 0.0).all() and (G[OUT] == 0.0).all(), name
        err = np.abs(H - G)
        m = E > 0
        ratio = float(np.max(err[m] / (EPS * E[m]))) if m.any() else 0.0
        assert (err <= ref.HELPER_BOUND * EPS * E).all(), (name, ratio)
        worst = max(worst, ratio)
    print(f"NumPy helper: worst |err| / (eps E) = {worst:.2f}  (bound {ref.HELPER_BOUND}, recorded {ref.HELPER_WORST_MEASURED}, device K = {ref.K_DEVICE})")


def test_host_lowering_and_evaluation_under_sanitizers(exact_blocks, tmp_path):
    """wendland_check.cpp: lower every case in C++, evaluate it through the evaluation core the device kernels run, on the host;
    every entry to K_DEVICE eps E, exactly 0 outside the support and wherever the tile decision says "out of reach", coincident
    entries equal to desc_diag; refusals; AddressSanitizer + UBSan."""
    import linpde_gp_amd as lp
    cf = lp.randprocs.covfuncs
    gxx = shutil.which(os.environ.get("CXX", "g++"))
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "wendland_check")
    clang = "clang" in subprocess.run([gxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static_rt, "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(CSRC, "hosttest", "wendland_check.cpp"), os.path.join(CSRC, "lower.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    rec = [float(len(exact_blocks))]
    for name, (kern, L0, L1, X0, X1, G, E, OUT) in exact_blocks.items():
        groups = cf.lower_groups(ref.base_groups(kern), L0, L1)
        d = groups[0]["d"]
        rec += [d, len(groups)]
        for g in groups:
            rec += [*g["family"], *g["p"], *g["lengthscale"], g["scale"], len(g["terms"])]
            for c, a, b in g["terms"]:
                rec += [c, *a, *b]
        # a coincident pair in every case: the diagonal value
        X1 = X1.copy()
        G, E, OUT = G.copy(), E.copy(), OUT.copy()
        X1[0] = X0[0]
        g0, e0, o0 = ref.exact_block(kern, L0, L1, X0, X1[:1])
        G[:, 0], E[:, 0], OUT[:, 0] = g0[:, 0], e0[:, 0], o0[:, 0]
        rec += [X0.shape[0], X1.shape[0], *X0.ravel(), *X1.ravel(), *G.ravel(), *E.ravel(), *OUT.astype(np.double).ravel()]
    path = str(tmp_path / "cases.bin")
    np.asarray(rec, dtype="<f8").tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe, path, repr(ref.K_DEVICE)], env=env, capture_output=True, text=True, timeout=300)
    print(res.stdout[-6000:])
    assert res.returncode == 0, res.stdout[-6000:] + "\n" + res.stderr[-4000:]
    assert "wendland_check: all checks passed" in res.stdout
    assert " 0 sub-blocks out of reach\n" not in res.stdout.splitlines(keepends=True)[-2], "the sorted cases must exercise the tile decision"
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr


def test_posterior_problem_lapack_vs_refined():
    """The posterior problem of tests/test_gpu_wendland.py: fp64 LAPACK against solves refined in long double, 1e-10 relative for the
    mean, the variance and the leave-one-out quantities -- the reference's own error, two orders below the 1e-8 the device is held to."""
    a, b = ref.posterior_lapack(), ref.posterior_refined()
    print(f"cond_2 = {a['cond']:.3e}")
    for key in ("mean", "var", "loo_mean", "loo_var"):
        rel = float(np.max(np.abs(a[key] - b[key])) / np.max(np.abs(b[key])))
        print(f"{key}: LAPACK vs refined {rel:.2e}")
        assert rel <= 1e-10, key
    assert np.isfinite(a["lml"]) and (a["var"] > -1e-12).all()
