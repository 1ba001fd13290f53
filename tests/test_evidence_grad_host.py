"""Host side of the evidence gradient: the descriptor field `lpgp_kdesc.dlog_lengthscale` and its lowering (csrc/lower.cpp), on the
CPU box.  The host-only code (lower.cpp + eval_entries.h behind csrc/hosttest/host_check.cpp) is compiled here with the host
compiler into a temporary library -- no sanitizer, no preload: `build.sh --host-asan` / tests/test_host_asan.py cover that.

* `_lib.KDesc` has the field and the size the C compiler gives `lpgp_kdesc`;
* a zero flag lowers to the bytes the lowering produced before the field existed (tests/golden/lowering_c1_c3.npz, recorded from
  that lowering), for the block descriptors of the 1-D (c1) and 2-D (c3) Poisson workloads;
* a flagged descriptor, evaluated by the evaluation core the GPU kernels use, is the derivative of the plain one by the log
  lengthscale: against a Richardson-extrapolated central difference of the plain descriptor over the lengthscale (Matern and
  ExpQuad factors, identity / first derivative / Laplacian on either side, 1-D and 2-D); `desc_diag` agrees with the block's
  entries at coinciding points; the isotropic Matern and an out-of-range flag are refused."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from linpde_gp_amd import _lib, problems
from linpde_gp_amd.randprocs import covfuncs as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linpde-gp_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lowering_c1_c3.npz")
pd = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("hostlib") / "liblpgp_hostcheck.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(CSRC, "lower.cpp"), os.path.join(CSRC, "options.cpp"), os.path.join(CSRC, "hosttest", "host_check.cpp"),
                    "-o", out], check=True)
    lib = C.CDLL(out)
    lib.lpgp_host_sizeof_kdesc.restype = C.c_int64
    lib.lpgp_host_lower_bytes.restype = C.c_int64
    lib.lpgp_host_lower_bytes.argtypes = [C.POINTER(_lib.KDesc), C.c_int32, C.c_char_p, C.c_int64]
    lib.lpgp_host_kernel_matrix.restype = C.c_int
    lib.lpgp_host_kernel_matrix.argtypes = [C.POINTER(_lib.KDesc), C.c_int32, pd, C.c_int64, pd, C.c_int64, pd]
    lib.lpgp_host_kernel_diag.restype = C.c_int
    lib.lpgp_host_kernel_diag.argtypes = [C.POINTER(_lib.KDesc), C.c_int32, pd]
    lib.lpgp_host_last_error.restype = C.c_char_p
    return lib


def lower_bytes(lib, groups) -> bytes:
    arr = _lib.make_kdesc_array(groups)
    need = lib.lpgp_host_lower_bytes(arr, len(arr), None, 0)
    assert need > 0, lib.lpgp_host_last_error()
    buf = C.create_string_buffer(need)
    assert lib.lpgp_host_lower_bytes(arr, len(arr), buf, need) == need
    return buf.raw


def host_matrix(lib, groups, X0, X1):
    arr = _lib.make_kdesc_array(groups)
    X0 = np.ascontiguousarray(X0, dtype=np.double).reshape(len(X0), -1)
    X1 = np.ascontiguousarray(X1, dtype=np.double).reshape(len(X1), -1)
    out = np.full((X0.shape[0], X1.shape[0]), np.nan)
    rc = lib.lpgp_host_kernel_matrix(arr, len(arr), _lib.as_pd(X0), X0.shape[0], _lib.as_pd(X1), X1.shape[0], _lib.as_pd(out))
    assert rc == 0, lib.lpgp_host_last_error()
    return out


def workload_descriptors():
    """name -> descriptor groups of every block pair of the 1-D (c1) and 2-D (c3) Poisson workloads: value x value, PDE x value, PDE x PDE."""
    out = {}
    for name, wl in (("c1", problems.poisson_1d(n=16, m=4)), ("c3", problems.poisson_2d(n_side=4, m_side=2))):
        prior = problems.build_prior(wl)
        d = max(int(np.prod(prior.input_shape, dtype=int)), 1)
        ident = {(0,) * d: 1.0}
        lap = {tuple(2 * int(i == j) for i in range(d)): -1.0 for j in range(d)}
        base = cf._base(prior.cov)
        for tag, (c0, c1) in {"vv": (ident, ident), "pv": (lap, ident), "pp": (lap, lap)}.items():
            out[f"{name}_{tag}"] = cf.DifferentiatedCovarianceFunction(base, c0, c1).lower()
    return out


def test_kdesc_has_the_field_and_the_c_size(host):
    names = [f[0] for f in _lib.KDesc._fields_]
    assert names[-1] == "dlog_lengthscale" and names[-2] == "terms"           # appended after `terms`
    assert C.sizeof(_lib.KDesc) == host.lpgp_host_sizeof_kdesc()
    arr = _lib.make_kdesc_array([{"d": 1, "family": [1], "p": [2], "lengthscale": [1.0], "scale": 1.0, "terms": [(1.0, (0,), (0,))]}])
    assert arr[0].dlog_lengthscale == 0                                          # a descriptor built without the key keeps its meaning
    with pytest.raises(ValueError):
        _lib.make_kdesc_array([{"d": 1, "family": [1], "p": [2], "lengthscale": [1.0], "scale": 1.0, "terms": [(1.0, (0,), (0,))],
                                "dlog_lengthscale": 2}])


def test_zero_flag_lowers_bit_identically_to_the_earlier_lowering(host):
    golden = np.load(GOLDEN)
    descs = workload_descriptors()
    assert sorted(golden.files) == sorted(descs)
    for name, groups in descs.items():
        assert all(g.get("dlog_lengthscale", 0) == 0 for g in groups)
        assert lower_bytes(host, groups) == golden[name].tobytes(), name


def richardson(f, h):
    """d f / d t at t = 0 from central differences with steps h and h / 2, the h^2 term removed (error O(h^4))."""
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(h / 2) - f(-h / 2)) / h
    return (4 * d2 - d1) / 3


CASES = []
for _nu in (1.5, 2.5):
    CASES.append((f"matern{_nu}", lambda l, nu=_nu: cf.Matern((), nu=nu, lengthscales=l[0]), 1, [0.7]))
CASES.append(("expquad", lambda l: 1.3 * cf.ExpQuad((), lengthscales=l[0]), 1, [0.45]))
CASES.append(("m52 x expquad", lambda l: 2.0 * cf.TensorProduct(cf.Matern((), nu=2.5, lengthscales=l[0]), cf.ExpQuad((), lengthscales=l[1])), 2, [0.8, 0.5]))
CASES.append(("m52 x m32", lambda l: cf.TensorProduct(cf.Matern((), nu=2.5, lengthscales=l[0]), cf.Matern((), nu=1.5, lengthscales=l[1])), 2, [1.1, 0.6]))


@pytest.mark.parametrize("name,make,d,ls", CASES, ids=[c[0] for c in CASES])
def test_flagged_lowering_is_the_log_lengthscale_derivative(host, name, make, d, ls):
    rng = np.random.default_rng(20261017)
    X0, X1 = rng.uniform(-1, 1, (23, d)), rng.uniform(-1, 1, (19, d))
    X1[:5] = X0[:5]                                                              # coinciding pairs
    ident = {(0,) * d: 1.0}
    first = {tuple(int(i == 0) for i in range(d)): 1.0}
    lap = {tuple(2 * int(i == j) for i in range(d)): -1.0 for j in range(d)}
    ops = [(ident, ident), (first, ident), (ident, first), (lap, ident), (ident, lap)]
    if "1.5" not in name and "m32" not in name:
        ops.append((lap, lap))                                                   # (a Matern-3/2 factor is not four times differentiable)
    else:
        ops.append((first, first))
    for c0, c1 in ops:
        for j in range(d):
            def plain(t, j=j):
                l = list(ls)
                l[j] = ls[j] * np.exp(t)
                return host_matrix(host, cf.DifferentiatedCovarianceFunction(cf._base(make(l)), c0, c1).lower(), X0, X1)
            groups = cf.DifferentiatedCovarianceFunction(cf._base(make(ls)), c0, c1).lower()
            got = host_matrix(host, [dict(g, dlog_lengthscale=j + 1) for g in groups], X0, X1)
            ref = richardson(plain, 2e-2)
            scale = max(np.max(np.abs(ref)), np.max(np.abs(plain(0.0))))
            # truncation h^4 f^(5) / 30 ~ 1e-8 f^(5) and rounding eps / h ~ 1e-14 of the block maximum
            assert np.max(np.abs(got - ref)) <= 2e-6 * scale, (name, c0, c1, j, np.max(np.abs(got - ref)) / scale)
            # desc_diag: the value at coinciding points
            arr = _lib.make_kdesc_array([dict(g, dlog_lengthscale=j + 1) for g in groups])
            v = C.c_double()
            assert host.lpgp_host_kernel_diag(arr, len(arr), C.byref(v)) == 0
            assert np.all(np.abs(np.diag(got)[:5] - v.value) <= 1e-13 * scale), (name, c0, c1, j)


def test_flag_refusals(host):
    k = cf.Matern((2,), nu=2.5, lengthscales=[0.7, 1.2])                         # isotropic
    groups = [dict(g, dlog_lengthscale=1) for g in k.lower()]
    arr = _lib.make_kdesc_array(groups)
    X = np.zeros((2, 2))
    out = np.zeros((2, 2))
    assert host.lpgp_host_kernel_matrix(arr, 1, _lib.as_pd(X), 2, _lib.as_pd(X), 2, _lib.as_pd(out)) != 0
    assert b"isotropic" in host.lpgp_host_last_error()
    arr = _lib.make_kdesc_array(cf.TensorProduct(cf.Matern((), nu=2.5), cf.Matern((), nu=2.5)).lower())
    for bad in (-1, 3):
        arr[0].dlog_lengthscale = bad
        assert host.lpgp_host_kernel_matrix(arr, 1, _lib.as_pd(X), 2, _lib.as_pd(X), 2, _lib.as_pd(out)) != 0
        assert b"dlog_lengthscale" in host.lpgp_host_last_error()
