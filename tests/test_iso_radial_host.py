"""Second-order operators on the isotropic Matern kernel (the radial family, `LPGP_MATERN_RADIAL`), the part that needs no GPU:
the NumPy helper against the 50-digit goldens (`tests/golden/iso_radial.npz`), the Python lowering with the flag off and on, and
the C++ lowering + the shared evaluation core on the host under AddressSanitizer / UBSan (`csrc/hosttest/radial_check.cpp`, a
stand-alone program run as a subprocess)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "linpde-gp_amd", "csrc")
sys.path.insert(0, HERE)
import _iso_radial_reference as ref  # noqa: E402

EPS = 2.0**-53
CASES = [(d, p) for d in (2, 3) for p in (2, 3, 4)]
OPS = ("lap_id", "id_lap", "lap_lap", "d01_lap", "mix_mix")


def operator_pairs(d, v):
    """The operator pairs of make_golden_iso_radial.py as {multi-index: coefficient} maps."""
    z = (0,) * d
    e = lambda i, k=1: tuple(k if j == i else 0 for j in range(d))  # noqa: E731
    ident = {z: 1.0}
    lap = {e(i, 2): 1.0 for i in range(d)}
    d01 = {tuple(1 if j < 2 else 0 for j in range(d)): 1.0}
    mix = {z: 2.0}
    for i in range(d):
        mix[e(i, 2)] = -0.5
        mix[e(i)] = float(v[i])
    return {"lap_id": (lap, ident), "id_lap": (ident, lap), "lap_lap": (lap, lap), "d01_lap": (d01, lap), "mix_mix": (mix, mix)}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "iso_radial.npz"))


def test_numpy_helper_vs_golden(golden):
    """|helper - G| <= HELPER_BOUND eps E for every entry; prints the worst ratio (the figure K_DEVICE = 4 x is derived from)."""
    worst = 0.0
    for d, p in CASES:
        tag = f"d{d}_nu{2 * p + 1}2"
        for name, (L0, L1) in operator_pairs(d, golden[tag + "_v"]).items():
            B = ref.block(p, golden[tag + "_lengthscales"], L0, L1, golden[tag + "_X0"], golden[tag + "_X1"])
            G, E = golden[f"{tag}_{name}"], golden[f"{tag}_{name}_E"]
            assert np.isfinite(B).all()
            err = np.abs(B - G)
            assert (err <= ref.HELPER_BOUND * EPS * E).all(), (tag, name, float(np.max(err[E > 0] / (EPS * E[E > 0]))))
            worst = max(worst, float(np.max(err[E > 0] / (EPS * E[E > 0]))))
    print(f"NumPy helper: worst |err| / (eps E) = {worst:.2f}  (bound {ref.HELPER_BOUND}, device K = {ref.K_DEVICE})")


def test_golden_limits_and_symmetry(golden):
    """Sanity of the vectors themselves: (Lap, id) = (id, Lap) for the symmetric kernel, and the 2-D bi-Laplacian of Matern-5/2 at
    coincident points is psi''(0) (3 a_0^4 + 2 a_0^2 a_1^2 + 3 a_1^4) with psi''(0) = 1 / 3 (8 / 3 for a_0 = a_1 = 1)."""
    for d, p in CASES:
        tag = f"d{d}_nu{2 * p + 1}2"
        np.testing.assert_allclose(golden[tag + "_lap_id"], golden[tag + "_id_lap"], rtol=1e-15, atol=0)
    a = np.sqrt(5.0) / golden["d2_nu52_lengthscales"]
    want = (1.0 / 3.0) * (3 * a[0]**4 + 2 * a[0]**2 * a[1]**2 + 3 * a[1]**4)
    np.testing.assert_allclose(golden["d2_nu52_lap_lap"][np.arange(4), np.arange(4)], want, rtol=1e-14)


def test_python_lowering_flag_off_refuses_flag_on_emits_radial():
    import linpde_gp_amd as lp
    from linpde_gp_amd import _lib
    from linpde_gp_amd.linfuncops import diffops
    cf = lp.randprocs.covfuncs
    assert lp.config.isotropic_matern_higher_order is False
    k = cf.Matern((2,), nu=2.5, lengthscales=[0.5, 2.0])
    lap = diffops.Laplacian((2,))
    with pytest.raises(NotImplementedError, match="TensorProduct"):
        lap(k, argnum=0).lower()
    first = diffops.DirectionalDerivative([1.0, -2.0])(k, argnum=1).lower()
    saved = lp.config.isotropic_matern_higher_order
    lp.config.isotropic_matern_higher_order = True
    try:
        (g,) = lap(lap(k, argnum=1), argnum=0).lower()
        assert g["family"] == [_lib.MATERN_RADIAL] * 2 and g["p"] == [2, 2] and g["lengthscale"] == [0.5, 2.0]
        assert sorted((c, tuple(a), tuple(b)) for c, a, b in g["terms"]) == sorted(
            (1.0, a, b) for a in ((2, 0), (0, 2)) for b in ((2, 0), (0, 2)))
        # first-order groups keep family 3 and their terms
        assert diffops.DirectionalDerivative([1.0, -2.0])(k, argnum=1).lower() == first
        assert first[0]["family"] == [_lib.MATERN_ISO] * 2
        # a sum of orders 0, 1, 2 is ONE radial group
        (g2,) = cf.lower_groups(k._base_groups(), {(0, 0): 2.0, (1, 0): 0.5, (1, 1): 1.0}, {(0, 0): 1.0})
        assert g2["family"] == [_lib.MATERN_RADIAL] * 2 and len(g2["terms"]) == 3
        with pytest.raises(ValueError, match="5/2"):
            lap(cf.Matern((2,), nu=1.5), argnum=0).lower()
        with pytest.raises(NotImplementedError, match="two derivatives"):
            cf.lower_groups(k._base_groups(), {(2, 1): 1.0}, {(0, 0): 1.0})
        # the C descriptor carries the family
        arr = _lib.make_kdesc_array(lap(k, argnum=0).lower())
        assert list(arr[0].family[:2]) == [4, 4]
    finally:
        lp.config.isotropic_matern_higher_order = saved


def test_host_lowering_and_evaluation_under_sanitizers(golden, tmp_path):
    """radial_check.cpp: lower every golden case in C++, evaluate it through the evaluation core the device kernels run, on the host,
    hold every entry to K_DEVICE eps E and the coincident entries to desc_diag exactly; refusals; AddressSanitizer + UBSan."""
    gxx = shutil.which(os.environ.get("CXX", "g++"))
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "radial_check")
    # the sanitizer runtimes are linked INTO the program, so that it does not care what else the environment loads before it
    clang = "clang" in subprocess.run([gxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static_rt, "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(CSRC, "hosttest", "radial_check.cpp"), os.path.join(CSRC, "lower.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    rec = [float(len(CASES) * len(OPS))]
    for d, p in CASES:
        tag = f"d{d}_nu{2 * p + 1}2"
        for name, (L0, L1) in operator_pairs(d, golden[tag + "_v"]).items():
            terms = [(c0 * c1, a, b) for a, c0 in L0.items() for b, c1 in L1.items()]
            rec += [d, p, *golden[tag + "_lengthscales"], len(terms)]
            for c, a, b in terms:
                rec += [c, *a, *b]
            rec += [24, 24, *golden[tag + "_X0"].ravel(), *golden[tag + "_X1"].ravel(), *golden[f"{tag}_{name}"].ravel(),
                    *golden[f"{tag}_{name}_E"].ravel()]
    path = str(tmp_path / "cases.bin")
    np.asarray(rec, dtype="<f8").tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe, path, repr(ref.K_DEVICE)], env=env, capture_output=True, text=True, timeout=300)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + "\n" + res.stderr[-4000:]
    assert "radial_check: all checks passed" in res.stdout
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr
