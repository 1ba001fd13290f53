"""The scattered-block reference of tests/_entry_reference.py, its bound model and its cases, checked on the CPU before the device
is held against them (tests/test_gpu_entry_exact.py):

* the reference agrees with `oracle.covfuncs.LkL` (and the golden first-order isotropic blocks with `_iso_radial_reference.block`)
  entry by entry within K / 4 -- the ratios these print are what K_ENTRY and K_ISO_FIRST are made of, and the figures recorded in
  `_entry_reference` are asserted to be the measured ones;
* the host instantiation of the evaluation core (`csrc/hosttest/entries_check.cpp`: lower_kdesc + eval_entries<D, 4> and <D, 8>, plain
  and through per-point factors, under AddressSanitizer + UBSan, a stand-alone program run as a subprocess) meets the bound on every
  entry of every case: the reference, the bound model (rho, eta) and the inputs hold without a GPU;
* a wrong kernel is visible: a sign forced to +1, an exchanged fastest dimension, a column taken one to the side, a column tile
  dropped from a product all miss the bound by orders of magnitude on every case that can show them.
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "linpde-gp_amd", "csrc")
sys.path.insert(0, HERE)

from oracle import covfuncs as ocf  # noqa: E402

import _entry_reference as er  # noqa: E402
import _iso_radial_reference as ir  # noqa: E402
from test_gpu_kron_exact import _covfunc, _operator  # noqa: E402

EPS, LD = er.EPS, er.LD
CASES = er.CASES
_measured = {}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_reference_against_the_oracle(case):
    B = case.reference()
    X0, X1 = case.points()
    assert np.all(np.isfinite(B.G.astype(np.double))) and np.all(B.E >= 0) and np.all(np.abs(B.G) <= B.E * (1 + 1e-15))
    ratio, pos = B.ratio(ocf.LkL(case.kernel, case.L0, case.L1, X0, X1), case.mask())
    i, j = divmod(pos, case.n1)
    print(f"rho_oracle {case.id}: {ratio / EPS:.2f} eps at ({i}, {j}), rho = {float(B.rho[i, j]):.3g}")
    _measured[case.id] = ratio
    assert ratio <= er.K_ENTRY / 4, (case.id, ratio / EPS, (i, j))
    if case.pset == "b":
        # the planted pairs are where they are meant to be
        k0 = er.PLANT if case.kind == "diag" else 0
        ex = lambda k: float(B.expo0[k0 + k, k])      # noqa: E731  (placed by the first group's scales)
        assert ex(0) == 0.0 and ex(2) < 1e-7 and ex(3) < 1e-3
        assert abs(ex(4) - er.T_NEAR) < 1e-6 and abs(ex(6) - er.T_FAR) < 1e-6 and 710 < ex(8) < 740 and ex(9) > 801
        assert float(B.eta[k0 + 8, 8]) > 0
        assert float(B.eta[k0 + 6, 6]) == 0.0 or len(case.kernel) > 1
        if case.D > 1:
            assert X0[k0 + 1, 0] == X1[1, 0] and np.all(X0[k0 + 1, 1:] != X1[1, 1:])
    if case.pset == "c" and case.factored:
        ok, bad = er.factor_tiles(case.kernel, X0, X1, lower=case.kind == "diag")
        assert ok >= 1 and bad >= 1, (ok, bad)


def test_the_recorded_k_entry_is_the_measured_one():
    """Runs behind the parametrised test above (file order): the maximum of its ratios is the figure in the module."""
    for c in CASES:
        if c.id not in _measured:            # (run on its own)
            _measured[c.id] = c.reference().ratio(ocf.LkL(c.kernel, c.L0, c.L1, *c.points()), c.mask())[0]
    worst = max(_measured, key=_measured.get)
    print(f"max rho_oracle = {_measured[worst] / EPS:.3f} eps, set by {worst}; K_ENTRY = {er.K_ENTRY / EPS:.2f} eps")
    assert abs(_measured[worst] - er.RHO_ORACLE_MAX) <= 0.005 * EPS, (worst, _measured[worst] / EPS)


def test_iso_first_helper_against_the_golden():
    """`_iso_radial_reference.block` against tests/golden/iso_first.npz within K_ISO_FIRST / 4; the recorded figure is the measured
    one; every case lowers to the first-order isotropic family (not the radial one); `iso_first_block` (the product cases' reference
    on other points) reproduces the file."""
    import linpde_gp_amd as lp
    from linpde_gp_amd import _lib
    cf = lp.randprocs.covfuncs
    worst, who = 0.0, None
    assert lp.config.isotropic_matern_higher_order is False
    cases = er.iso_first_cases()
    assert len(cases) == 2 * (1 + 3 + 5 + 5)
    for cid, d, p, ls, L0, L1, X0, X1, B in cases:
        ratio, pos = B.ratio(ir.block(p, ls, L0, L1, X0, X1))
        print(f"rho_helper {cid}: {ratio / EPS:.2f} eps at {divmod(pos, 24)}, s = {float(B.rho.reshape(-1)[pos]):.3g}")
        assert ratio <= er.K_ISO_FIRST / 4, (cid, ratio / EPS)
        if ratio > worst:
            worst, who = ratio, cid
        groups = _operator(L0)(_operator(L1)(cf.Matern((d,), nu=p + 0.5, lengthscales=ls), argnum=1), argnum=0).lower()
        assert len(groups) == 1 and groups[0]["family"] == [_lib.MATERN_ISO] * d, cid
        # the layout of the file: coincident pairs, 1e-9 and 1e-5 of a lengthscale, s ~ 50
        s = B.rho.astype(np.double)
        assert np.all(s[np.arange(4), np.arange(4)] == 0) and np.all(s[np.arange(4, 8), np.arange(4, 8)] < 1e-8)
        assert np.all(s[np.arange(8, 12), np.arange(8, 12)] < 1e-4) and np.all(np.abs(s[np.arange(12, 16), np.arange(12, 16)] - 50) < 1e-6)
    print(f"max rho_helper = {worst / EPS:.3f} eps, set by {who}; K_ISO_FIRST = {er.K_ISO_FIRST / EPS:.2f} eps")
    assert abs(worst - er.RHO_HELPER_MAX) <= 0.005 * EPS, (who, worst / EPS)
    # grad_grad has v != w: the matrix of the mixed term is not symmetric by accident
    for cid, d, p, ls, L0, L1, X0, X1, B in cases:
        if cid.endswith("grad_grad"):
            v, w = np.array([L0[k] for k in sorted(L0)]), np.array([L1[k] for k in sorted(L1)])
            assert np.max(np.abs(np.outer(v, w) - np.outer(w, v))) > 0.1
    for cid, d, p, ls, L0, L1, X0, X1, B in (cases[7], cases[-1]):
        B2 = er.iso_first_block(p, ls, L0, L1, X0, X1)
        # (the file's lengthscales are the decimal fractions, these the float64 ones: 2e-17 relative, times s in the exponent)
        assert np.all(np.abs(B2.G - B.G) <= EPS * B.W), cid
        assert np.all(np.abs(B2.E - B.E) <= 2e-7 * B.E), cid


def _kdesc_record(groups):
    rec = [groups[0]["d"], len(groups)]
    for g in groups:
        rec += [*g["family"], *g["p"], *g["lengthscale"], g["scale"], len(g["terms"])]
        for c, a, b in g["terms"]:
            rec += [c, *a, *b]
    return rec


def test_host_instantiation_under_sanitizers(tmp_path):
    """entries_check.cpp: every case lowered in C++ and evaluated through the evaluation core the device kernels run, on the host,
    every entry to K W + eta, exactly 0 beyond the clamp; the lowered shapes agree with the restated kernel choice."""
    import linpde_gp_amd as lp
    cf = lp.randprocs.covfuncs
    gxx = shutil.which(os.environ.get("CXX", "g++"))
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "entries_check")
    clang = "clang" in subprocess.run([gxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static_rt, "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(CSRC, "hosttest", "entries_check.cpp"), os.path.join(CSRC, "lower.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    assert np.dtype(LD).itemsize == 16, "the reference file is written as this platform's 16-byte long double"
    rec, ref, ids = [], [], []

    def add(which, lower, groups, X0, X1, B):
        rec.extend([which, lower, *_kdesc_record(groups), X0.shape[0], X1.shape[0], *X0.ravel(), *X1.ravel()])
        zero = (B.expo > er.EXP_CLAMP + 1).astype(LD)
        ref.extend([B.G.ravel(), B.W.ravel(), B.eta.ravel(), zero.ravel()])

    for c in CASES:
        X0, X1 = c.points()
        groups = _operator(c.L0)(_operator(c.L1)(_covfunc(lp, c.kernel), argnum=1), argnum=0).lower()
        add(0, int(c.kind == "diag"), groups, X0, X1, c.reference())
        ids.append(c.id)
    for cid, d, p, ls, L0, L1, X0, X1, B in er.iso_first_cases():
        add(1, 0, _operator(L0)(_operator(L1)(cf.Matern((d,), nu=p + 0.5, lengthscales=ls), argnum=1), argnum=0).lower(), X0, X1, B)
        ids.append(cid)
    np.asarray([float(len(ids)), *rec], dtype="<f8").tofile(str(tmp_path / "cases.bin"))
    np.concatenate(ref).astype(LD).tofile(str(tmp_path / "ref.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "ref.bin"), repr(er.K_ENTRY), repr(er.K_ISO_FIRST)], env=env,
                         capture_output=True, text=True, timeout=600)
    lines = res.stdout.splitlines()
    for cid, line in zip(ids, lines):
        print(cid, "|", line)
    print("\n".join(lines[len(ids):]))
    assert res.returncode == 0, res.stdout[-6000:] + "\n" + res.stderr[-4000:]
    assert "entries_check: all checks passed" in res.stdout
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr
    # both kinds of strip occurred: with the per-point factors and falling back
    m = re.search(r"^strips with factors (\d+), without (\d+)$", res.stdout, re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0
    # the lowered shape of every product-form case is what `fast_instantiation` restates
    for c, line in zip(CASES, lines):
        m = re.search(r"groups=(\d+) iso=(\d+) ncls=(\d+) deg=(\d+),(\d+),\d+,\d+ parity=(\d+),(\d+) kinds=(\d+),(\d+)", line)
        ng, iso, ncls, d0, d1, p0, p1, k0, k1 = map(int, m.groups())
        fast = er.fast_instantiation(c.kernel, c.L0, c.L1)
        lowered = None
        if c.D <= 2 and ng == 1 and not iso and ncls <= 2 and d0 <= 4 and (c.D == 1 or d1 <= 4):
            N0, N1 = d0 + 1, (d1 + 1 if c.D == 2 else 1)
            if ncls * N0 * N1 <= 32:
                kinds = (k0, k1)[:c.D]
                mask = (1 << c.D) - 1
                lowered = (N0, N1, 0 if any(k != 1 for k in kinds) else (1 if ((p0 | (p1 if ncls > 1 else 0)) & mask) else 2))
        assert fast == lowered, (c.id, fast, lowered, line)
        assert er.kernel_name(c.kernel, c.L0, c.L1) == c.expected, c.id
    for cid, line in zip(ids[len(CASES):], lines[len(CASES):]):
        assert " iso=1 " in line and "groups=1 " in line, (cid, line)


def test_the_cases_cover_the_instantiations_named_in_the_plan():
    names = {c.expected for c in CASES}
    for mode in (0, 1, 2):
        assert any(re.fullmatch(rf"assemble_fast<1,\d,1,{mode}>", n) for n in names), mode
        assert any(re.fullmatch(rf"assemble_fast<2,\d,\d,{mode}>", n) for n in names), mode
    sizes = {tuple(map(int, re.findall(r"\d", n)[1:3])) for n in names if n.startswith("assemble_fast<2")}
    assert {(1, 1), (1, 3), (5, 1), (3, 5), (5, 3), (1, 5), (3, 3)} <= sizes, sizes
    assert {"assemble<2,->", "assemble<3,->", "assemble<4,->"} <= names
    shapes = {(c.kind, c.n0, c.n1) for c in CASES}
    assert {("off", 1, 1), ("off", 64, 64), ("off", 65, 150), ("off", 130, 17), ("diag", 130, 130)} <= shapes
    assert all(c.n0 * c.n1 <= er.MAX_ENTRIES for c in CASES)
    # an odd order in the fastest dimension wherever the instantiation allows one
    for c in CASES:
        fast = er.fast_instantiation(c.kernel, c.L0, c.L1)
        even_by_design = (fast is not None and fast[2] == 2) or c.desc in ("s1-q1", "s2-51-odd")
        assert even_by_design or (c.D - 1) in c.odd_dims(), c.id


WIDE = [c for c in CASES if c.n0 * c.n1 > 1]      # (a block of one entry has no neighbour, and one pair shows a sign or not)


@pytest.mark.parametrize("case", WIDE, ids=[c.id for c in WIDE])
def test_a_wrong_kernel_is_visible(case):
    """Asserted on the reference: the wrong block misses K W + eta by more than 1e6 K W on some checked entry.
    * every dimension with an odd derivative order: its sign forced to +1;
    * rows and columns exchanged in the fastest dimension -- where the operators have an odd order there; on a descriptor that is
      even in the fastest dimension (MODE 2, nu = 1/2 there) the exchange is the identity of a stationary kernel, and the case
      must see the fastest factor taken one column to the side instead, which every case with more than one point is held to."""
    B = case.reference()
    mask = case.mask()
    K = er.K_ENTRY

    def missed(wrong):
        ratio, _ = B.ratio(wrong.G.astype(np.double), mask)
        return ratio
    for d in case.odd_dims():
        seen = missed(case.reference(plus_dim=d))
        assert seen > 1e6 * K, f"{case.id}: forcing the sign of dimension {d} to +1 moves no checked entry by more than {seen:.2e} W"
    if (case.D - 1) in case.odd_dims():
        seen = missed(case.reference(flip_dim=case.D - 1))
        assert seen > 1e6 * K, f"{case.id}: exchanging rows and columns in the fastest dimension moves no checked entry by more than {seen:.2e} W"
    seen = missed(case.reference(roll=True))
    assert seen > 1e6 * K, f"{case.id}: a fastest factor one column to the side moves no checked entry by more than {seen:.2e} W"


_small = {}


def small_block(desc):
    if desc not in _small:
        _small[desc] = er.small_product_block(desc)
    return _small[desc]


@pytest.mark.parametrize("name,desc,factors", er.PRODUCT_SMALL, ids=[p[0] for p in er.PRODUCT_SMALL])
def test_a_dropped_column_tile_is_visible_small(name, desc, factors):
    X0, X1, B = small_block(desc)
    n0, n1 = er.PRODUCT_SHAPE
    tiles_r, tiles_c, splits, per, owned = er.split_plan(n0, n1, 256)
    K = er.K_ISO_FIRST if desc == "iso" else er.K_ENTRY
    for m in er.PRODUCT_RHS:
        V = np.random.default_rng(m).standard_normal((n1, m))
        y, bound = er.product_reference(B, V, K, per, splits)
        assert np.all(bound > 0) and np.all(np.isfinite(y.astype(np.double)))
        Vd = V.copy()
        Vd[64:128] = 0.0
        miss = np.abs(B.G @ Vd.astype(LD) - y) / bound
        assert np.all(miss > 1e3), (name, m, float(miss.min()))


@pytest.mark.parametrize("desc", er.PRODUCT_BIG_DESCRIPTORS)
@pytest.mark.parametrize("name", [c[0] for c in er.PRODUCT_BIG])
def test_a_dropped_column_tile_is_visible_big(name, desc):
    """At the shapes a 256-CU device gets: the plan (splits, per, tiles per split) is the one the case is about, and the product
    without the columns [64, 128) -- the second tile of the first split -- misses every sampled row's bound by more than 1e3."""
    _, n0_of, n1, (splits_w, per_w, owned_w) = next(c for c in er.PRODUCT_BIG if c[0] == name)
    tiles_r, tiles_c, splits, per, owned = er.split_plan(n0_of(256), n1, 256)
    assert (splits, per, owned) == (splits_w, per_w, owned_w)
    X0, X1, V, rows, B = er.big_product(name, desc)
    assert len(rows) >= er.BIG_ROWS and {0, 63, 64, n0_of(256) - 1} <= set(rows.tolist())
    y, bound = er.product_reference(B, V, er.K_ENTRY, per, splits)
    Vd = V.copy()
    Vd[64:128] = 0.0
    miss = np.abs(B.G @ Vd.astype(LD) - y) / bound
    assert np.all(miss > 1e3), (name, desc, float(miss.min()))
