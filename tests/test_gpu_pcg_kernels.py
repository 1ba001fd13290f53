"""The kernels of `csrc/pcg.hip` -- device-resident vector blocks, the three-kernel preconditioner, the column dots and scalars of
`lpgp_pcg_start` / `lpgp_pcg_step`, `lpgp_kernel_matvec_dev` -- each against a reference of ITS OWN operation, not through a
converged solve (conjugate gradients correct themselves: a wrong preconditioner, a dropped partial sum or a wrong beta still
converges, only later).

The reference and every tolerance are tests/_pcg_reference.py: exact dots, `np.longdouble` vectors, and running error bounds
derived from the summation depths of the kernels (checked on the CPU by tests/test_pcg_reference.py).  No tolerance below is a
literal: each is such a bound, or equality bit for bit.  The one exception is the 1e-8 of the 257-column solve, the project's
posterior bar.  The iteration tests never run the kernel product: A V = d o V + W^T (W V) is applied on the host to `P.get()` and
written into Q, so n = 40 001 costs nothing.  The guards are asserted exactly, and what they pin is the HOST loop
`randprocs/_matrix_free.pcg`.  Every test prints its worst error / bound ratio (MEASUREMENTS.md, "PCG kernels against a reference")."""
import functools

import numpy as np
import pytest

import _pcg_reference as pr

pytestmark = pytest.mark.gpu

LD = pr.LD
RTOL = 1e-12


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


def bits(A):
    return np.ascontiguousarray(A, dtype=np.double).view(np.uint64)


def same_bits(A, B):
    return np.array_equal(bits(A), bits(B))


def sentinel(rng, shape):
    """values of every magnitude and sign, with -0.0, a subnormal and the largest finite number among them"""
    A = rng.standard_normal(shape) * 2.0 ** rng.integers(-40, 40, shape)
    flat = A.reshape(-1)
    flat[:: 7] = np.resize([-0.0, 5e-324, np.finfo(np.double).max, -1.0], flat[:: 7].shape)
    return A


# ---- (a) storage ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_set_get_round_trip_is_bit_identical(ctx, n, m):
    from linpde_gp_amd import _engine
    A = sentinel(np.random.default_rng(n + m), (n, m))
    D = _engine.DeviceVectors(ctx, n, m, A)
    assert same_bits(D.get(), A)
    E = _engine.DeviceVectors(ctx, n, m)
    assert same_bits(E.get(), np.zeros((n, m)))
    E.set(A[::-1])
    assert same_bits(E.get(), A[::-1]) and same_bits(D.get(), A)


@pytest.mark.parametrize("alias", ["none", "a", "b"])
def test_axpby_is_one_fma_per_element(ctx, alias):
    """out = a + s b is `fma(s, b, a)`: bit for bit against rational arithmetic, also where out is a or b; n = 257 is two workgroups
    with a ragged tail, and the padding rows of the 320-row block stay out of it."""
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(21)
    n, m, s = 257, 3, -0.7310585786300049
    A, B = rng.standard_normal((n, m)), rng.standard_normal((n, m)) * 2.0 ** rng.integers(-3, 4, (n, m))
    want = pr.fma_exact(s, B, A)
    assert np.any(want != A + s * B)                  # (the twice-rounded value differs somewhere: the check sees a mul + add)
    a, b = _engine.DeviceVectors(ctx, n, m, A), _engine.DeviceVectors(ctx, n, m, B)
    out = {"none": _engine.DeviceVectors(ctx, n, m, sentinel(rng, (n, m))), "a": a, "b": b}[alias]
    out.axpby(a, b, s)
    assert same_bits(out.get(), want)
    if alias != "a":
        assert same_bits(a.get(), A)
    if alias != "b":
        assert same_bits(b.get(), B)


@pytest.mark.parametrize("off,length", [(0, 65), (1, 256), (70, 129), (70, 263)])
def test_scale_rows_add_touches_its_rows_only(ctx, off, length):
    """Y[off : off + len] += diag(d) V[off : off + len]: the rows are `fma(d, V, Y)` bit for bit, every other row keeps its bits."""
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(off + length)
    n, m = 333, 3
    assert off + length <= n
    Y0, V0 = sentinel(rng, (n, m)), rng.standard_normal((n, m))
    Y0[off:off + length] = rng.standard_normal((length, m))
    d = rng.uniform(0.5, 2.0, length)
    Y, V = _engine.DeviceVectors(ctx, n, m, Y0), _engine.DeviceVectors(ctx, n, m, V0)
    Y.scale_rows_add(off, V, d)
    got = Y.get()
    rows = slice(off, off + length)
    assert same_bits(got[rows], pr.fma_exact(d[:, None], V0[rows], Y0[rows]))
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    assert same_bits(got[keep], Y0[keep]) and same_bits(V.get(), V0)


# ---- (b) the preconditioner -------------------------------------------------------------------------------------------------------
PRECOND_M = 5


@functools.lru_cache(maxsize=None)
def _precond_reference(n, rank):
    """one reference per (n, rank), with 5 columns; the one-column case is its first column"""
    pb = pr.problem(n, PRECOND_M, rank, symmetric=False)
    st, bd = pr.start(pb.preconditioner(), pb.B, pr.bnorm(pb.B), RTOL)
    for v in (st.Z, st.rel, bd["Z"], bd["rel"], pb.B):
        v.setflags(write=False)
    return pb, st, bd


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 40001])
@pytest.mark.parametrize("rank", [0, 1, 5, 64, 65])
def test_preconditioner_against_the_reference(ctx, rank, n, m):
    """`start()` leaves Z = M^-1 R: pcg_lr_kernel (256-stride loop: n = 255, 256, 257, 40 001), pcg_small_kernel (64-thread blocks:
    rank 64, 65) with a NON-SYMMETRIC S (a transposed index is off by the size of the correction), pcg_z_kernel; P == Z bit for bit;
    rel = ||R|| / bn from the column dots."""
    from linpde_gp_amd import _engine
    pb, st, bd = _precond_reference(n, rank)
    if rank > 1:
        assert np.max(np.abs(pb.S - pb.S.T)) > 0.1 * np.max(np.abs(pb.S))
    B = np.ascontiguousarray(pb.B[:, :m])
    R, Z, P = _engine.DeviceVectors(ctx, n, m, B), _engine.DeviceVectors(ctx, n, m), _engine.DeviceVectors(ctx, n, m)
    it = _engine.DevicePCG(ctx, n, m, pb.L if rank else None, pb.S if rank else None, pb.delta)
    rel = it.start(R, Z, P, pr.bnorm(pb.B)[:m], RTOL)
    Zh = Z.get()
    rz, rrel = pr.worst_ratio(Zh, st.Z[:, :m], bd["Z"][:, :m]), pr.worst_ratio(rel, st.rel[:m], bd["rel"][:m])
    print(f"preconditioner rank={rank} n={n} m={m}: error / bound Z {rz:.3f}, rel {rrel:.3f}")
    assert np.isfinite(Zh).all() and rz <= 1.0, rz
    assert same_bits(P.get(), Zh)
    assert rrel <= 1.0, rrel
    assert same_bits(R.get(), B)


# ---- (c) one step: local error ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,rank", pr.STEP_SHAPES, ids=[f"{n}x{m}-rank{r}" for n, m, r in pr.STEP_SHAPES])
def test_each_step_against_the_reference_from_the_device_state(ctx, n, m, rank):
    """Three steps; before each, X, R, Z, P are read back and the reference takes ONE step from that state (rz recomputed accurately
    from the device's R and Z: the stored rz is within the dot bound of it, which the tolerance carries).  So every step is judged on
    its own: no error of an earlier step is forgiven or accumulated.  n = 32 769 and 40 001 take the second trip of the dots'
    grid-stride loop, m = 256 fills the scalar kernel's workgroup."""
    from linpde_gp_amd import _engine
    pb = pr.problem(n, m, rank)
    pre, bn = pb.preconditioner(), pr.bnorm(pb.B)
    DV = _engine.DeviceVectors
    X, R, Z, P, Q = DV(ctx, n, m), DV(ctx, n, m, pb.B), DV(ctx, n, m), DV(ctx, n, m), DV(ctx, n, m)
    it = _engine.DevicePCG(ctx, n, m, pb.L, pb.S, pb.delta)
    rel = it.start(R, Z, P, bn, RTOL)
    worst = {}
    cond = 0.0
    for k in range(pr.STEPS):
        Xh, Rh, Zh, Ph = X.get(), R.get(), Z.get(), P.get()
        Qh = pb.matvec(Ph)
        Q.set(Qh)
        st = pr.state(pre, Xh, Rh, Zh, Ph, bn, RTOL)
        assert np.all(st.rz > 0) and np.all(st.active) and np.all(rel > RTOL)
        new, bd = pr.step(pre, st, Qh, RTOL)
        rel = it.step(X, R, Z, P, Q, RTOL)
        got = {"X": X.get(), "R": R.get(), "Z": Z.get(), "P": P.get(), "rel": rel}
        for key, g in got.items():
            assert np.isfinite(g).all(), key
            worst[key] = max(worst.get(key, 0.0), pr.worst_ratio(g, getattr(new, key), bd[key]))
        cond = max(cond, *(float(np.max(v)) for v in st.cond.values()), *(float(np.max(v)) for v in new.cond.values()))
        assert same_bits(Q.get(), Qh)
    print(f"step n={n} m={m} rank={rank}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; worst condition number of a dot {cond:.2f}")
    assert cond <= pr.COND_MAX, cond          # (an ill-conditioned draw fails here; it does not widen a bound)
    for key, v in worst.items():
        assert v <= 1.0, (key, v)


# ---- (d) guards: exactly the host loop ----------------------------------------------------------------------------------------------
def _iteration(ctx, pb, X0, R0, bn, rtol):
    from linpde_gp_amd import _engine
    DV = _engine.DeviceVectors
    n, m = R0.shape
    vec = dict(X=DV(ctx, n, m, X0), R=DV(ctx, n, m, R0), Z=DV(ctx, n, m), P=DV(ctx, n, m), Q=DV(ctx, n, m))
    it = _engine.DevicePCG(ctx, n, m, pb.L if pb.rank else None, pb.S if pb.rank else None, pb.delta)
    rel = it.start(vec["R"], vec["Z"], vec["P"], bn, rtol)
    return it, vec, rel


def _step(it, vec, rtol):
    return it.step(vec["X"], vec["R"], vec["Z"], vec["P"], vec["Q"], rtol)


@pytest.mark.parametrize("how", ["small_residual", "zero_column"])
def test_a_converged_column_is_frozen(ctx, how):
    """rel <= rtol at the start -- a residual 1e-14 of its right-hand side next to columns still to be solved; B[:, c] = 0 with
    bn = 1 -- : over two steps X and R of the column keep their bits and P == Z, while the other columns move."""
    n, m, c, rtol = 257, 3, 1, 1e-10
    pb = pr.problem(n, m, 3)
    rng = np.random.default_rng(2)
    X0, R0 = rng.standard_normal((n, m)), pb.B.copy()
    if how == "small_residual":
        bn = pr.bnorm(pb.B)
        R0[:, c] *= 1e-14
    else:
        R0[:, c] = 0.0
        bn = pr.bnorm(R0)
        assert bn[c] == 1.0
    it, vec, rel = _iteration(ctx, pb, X0, R0, bn, rtol)
    assert rel[c] <= rtol and np.all(np.delete(rel, c) > rtol)
    if how == "zero_column":
        assert rel[c] == 0.0
    Z0 = vec["Z"].get()
    others = [j for j in range(m) if j != c]
    for _ in range(2):
        before = {k: v.get() for k, v in vec.items()}
        vec["Q"].set(pb.matvec(before["P"]))
        rel_new = _step(it, vec, rtol)
        after = {k: v.get() for k, v in vec.items()}
        assert all(np.isfinite(v).all() for v in after.values()) and np.isfinite(rel_new).all()
        assert same_bits(after["X"][:, c], X0[:, c]) and same_bits(after["R"][:, c], R0[:, c])
        assert same_bits(after["Z"][:, c], Z0[:, c]) and same_bits(after["P"][:, c], after["Z"][:, c])
        assert rel_new[c] == rel[c]
        for j in others:
            assert np.any(after["X"][:, j] != before["X"][:, j]) and np.any(after["R"][:, j] != before["R"][:, j])
            assert np.any(after["P"][:, j] != after["Z"][:, j])


def test_a_column_without_positive_curvature_takes_no_step_and_restarts(ctx):
    """pq <= 0 (Q = -P in one column, Q = 0 in another): alpha = 0, so X and R keep their bits, and -- the HOST loop's semantics,
    `active = (rel > rtol) & (pq > 0)` -- beta = 0: P == Z after the step, not Z + P.  Everything stays finite."""
    n, m, rtol = 257, 4, RTOL
    pb = pr.problem(n, m, 3)
    rng = np.random.default_rng(3)
    X0 = rng.standard_normal((n, m))
    it, vec, rel = _iteration(ctx, pb, X0, pb.B, pr.bnorm(pb.B), rtol)
    assert np.all(rel > rtol)
    vec["Q"].set(pb.matvec(vec["P"].get()))
    _step(it, vec, rtol)                                   # an ordinary step first: P != Z from here on
    before = {k: v.get() for k, v in vec.items()}
    assert np.all(np.any(before["P"] != before["Z"], axis=0))
    Qh = pb.matvec(before["P"])
    Qh[:, 1] = -before["P"][:, 1]
    Qh[:, 2] = 0.0
    vec["Q"].set(Qh)
    rel_new = _step(it, vec, rtol)
    after = {k: v.get() for k, v in vec.items()}
    assert all(np.isfinite(v).all() for v in after.values()) and np.isfinite(rel_new).all()
    for c in (1, 2):
        assert same_bits(after["X"][:, c], before["X"][:, c]) and same_bits(after["R"][:, c], before["R"][:, c])
        assert same_bits(after["Z"][:, c], before["Z"][:, c])
        assert same_bits(after["P"][:, c], after["Z"][:, c]), "a column with pq <= 0 keeps its old direction (beta != 0)"
    for c in (0, 3):
        assert np.any(after["X"][:, c] != before["X"][:, c]) and np.any(after["P"][:, c] != after["Z"][:, c])
    # the host loop on the same state does the same
    st = pr.state(pb.preconditioner(), before["X"], before["R"], before["Z"], before["P"], pr.bnorm(pb.B), rtol)
    new, bd = pr.step(pb.preconditioner(), st, Qh, rtol)
    assert np.array_equal(new.beta[[1, 2]], [0, 0]) and np.array_equal(new.alpha[[1, 2]], [0, 0])
    for key in ("X", "R", "Z", "P"):
        assert pr.worst_ratio(after[key], getattr(new, key), bd[key]) <= 1.0, key


def test_a_zero_residual_makes_no_nan(ctx):
    """R = 0 in a column: rel == 0 and nothing is NaN, through `start` and two steps -- also when the column is kept ACTIVE (rtol < 0)
    with a direction put there by hand, so that pq > 0 and the division rz' / rz meets rz == 0."""
    n, m = 130, 3
    pb = pr.problem(n, m, 2)
    R0 = pb.B.copy()
    R0[:, 1] = 0.0
    for rtol in (RTOL, -1.0):
        it, vec, rel = _iteration(ctx, pb, np.zeros((n, m)), R0, pr.bnorm(R0), rtol)
        assert rel[1] == 0.0 and np.isfinite(rel).all()
        assert not vec["Z"].get()[:, 1].any() and not vec["P"].get()[:, 1].any()
        for k in range(2):
            Ph = vec["P"].get()
            if rtol < 0 and k == 0:
                Ph[:, 1] = pb.B[:, 1]
                vec["P"].set(Ph)
            vec["Q"].set(pb.matvec(Ph))
            rel = _step(it, vec, rtol)
            got = {key: v.get() for key, v in vec.items()}
            assert all(np.isfinite(v).all() for v in got.values()), (rtol, k)
            assert rel[1] == 0.0 and np.isfinite(rel).all()
            assert not got["X"][:, 1].any() and not got["R"][:, 1].any() and not got["Z"][:, 1].any() and not got["P"][:, 1].any()
            assert np.all(np.any(got["X"][:, [0, 2]] != 0.0, axis=0))


def test_refusals(ctx):
    """Argument checks, made before any launch: more columns than the scalar kernel's one workgroup, and blocks of another n -- also
    where the padded leading dimension (128 for n = 100 and for n = 120) is the same."""
    from linpde_gp_amd import _engine, _lib
    DV = _engine.DeviceVectors
    _engine.DevicePCG(ctx, 100, 256, None, None, 1.0)
    with pytest.raises(_lib.LpgpError):
        _engine.DevicePCG(ctx, 100, 257, None, None, 1.0)
    n, m = 100, 2
    it = _engine.DevicePCG(ctx, n, m, None, None, 1.0)
    good = lambda: DV(ctx, n, m, np.ones((n, m)))           # noqa: E731
    bn = np.ones(m)
    for bad in (DV(ctx, 120, m), DV(ctx, n, m + 1), DV(ctx, 200, m)):
        with pytest.raises(_lib.LpgpError):
            it.start(bad, good(), good(), bn, RTOL)
        with pytest.raises(_lib.LpgpError):
            it.start(good(), bad, good(), bn, RTOL)
        with pytest.raises(_lib.LpgpError):
            it.start(good(), good(), bad, bn, RTOL)
        assert same_bits(bad.get(), np.zeros((bad.n, bad.m)))            # (refused before anything was written)
    X, R, Z, P, Q = (good() for _ in range(5))
    it.start(R, Z, P, bn, RTOL)
    for bad in (DV(ctx, 120, m), DV(ctx, n, m + 1)):
        for pos in range(5):
            args = [X, R, Z, P, Q]
            args[pos] = bad
            with pytest.raises(_lib.LpgpError):
                it.step(*args, RTOL)
    Q.set(np.ones((n, m)))
    assert np.isfinite(it.step(X, R, Z, P, Q, RTOL)).all()


def test_more_than_256_columns_take_the_host_loop(ctx):
    """`gram.solve` with 257 right-hand sides at n = 200: beyond the scalar kernel's workgroup the solve runs the host loop
    (no "device_resident" in `last_solve_info`) and agrees with the dense solve to the posterior bar; 256 columns, the most the
    device-resident loop takes, do the same on the device."""
    import linpde_gp_amd as lp
    from conftest import POSTERIOR_RTOL
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(6)
    n = 200
    Xo, Y = rng.uniform(-1, 1, (n, 2)), rng.standard_normal(n)
    k = cf.TensorProduct(cf.Matern((), nu=2.5, lengthscales=0.5), cf.Matern((), nu=2.5, lengthscales=0.6))
    prior = lp.GaussianProcess(lp.functions.Zero((2,)), k)
    Bm = rng.standard_normal((n, 257))
    saved = (lp.config.matrix_free, lp.config.matrix_free_rtol, lp.config.matrix_free_device_iteration)
    lp.config.matrix_free, lp.config.matrix_free_rtol, lp.config.matrix_free_device_iteration = True, 1e-13, True
    try:
        u = prior.condition_on_observations(Y, Xo, b=lp.randvars.Normal(np.zeros(n), np.full(n, 1e-2)))
        S256 = u.gram.solve(Bm[:, :256])
        assert u.last_solve_info.get("device_resident") is True
        S = u.gram.solve(Bm)
        info = u.last_solve_info
    finally:
        lp.config.matrix_free, lp.config.matrix_free_rtol, lp.config.matrix_free_device_iteration = saved
    assert "device_resident" not in info and info["converged"]
    want = np.linalg.solve(k.matrix(Xo, Xo) + 1e-2 * np.eye(n), Bm)
    assert np.max(np.abs(S - want)) <= POSTERIOR_RTOL * np.max(np.abs(want))
    assert np.max(np.abs(S256 - want[:, :256])) <= POSTERIOR_RTOL * np.max(np.abs(want))


# ---- (e) the product on resident blocks against the host-vector path ------------------------------------------------------------------
MV_N, MV_N0, MV_N1 = 333, 130, 70
MV_OFFSETS = [(0, 0), (1, 70), (263, 203)]           # (v_off, y_off): none, neither, both beyond the first 64-row tile and ragged
MV_COLUMNS = [1, 4, 5, 9]                            # MV_RHS = 4 ride per pass: one pass, a full one, one + a rest, two + a rest


def _descriptor(name):
    import linpde_gp_amd as lp
    cf = lp.randprocs.covfuncs
    m52 = lambda ls: cf.Matern((), nu=2.5, lengthscales=ls)          # noqa: E731
    if name in ("product2d", "product2d_factors"):
        return 2, (1.3**2 * cf.TensorProduct(m52(0.5), m52(0.7))).lower()
    if name == "sum2d":
        return 2, (cf.TensorProduct(m52(0.5), m52(0.7)) + 0.5 * cf.TensorProduct(cf.Matern((), nu=1.5, lengthscales=0.9), cf.ExpQuad((), lengthscales=0.6))).lower()
    if name == "product3d":
        return 3, cf.TensorProduct(m52(0.5), cf.ExpQuad((), lengthscales=0.8), cf.Matern((), nu=1.5, lengthscales=0.7)).lower()
    assert name == "radial2d"
    saved = lp.config.isotropic_matern_higher_order
    lp.config.isotropic_matern_higher_order = True
    try:
        lap, ident = {(2, 0): 1.0, (0, 2): 1.0}, {(0, 0): 1.0}
        desc = cf.lower_groups(cf.Matern((2,), nu=2.5, lengthscales=[0.8, 0.6])._base_groups(), lap, ident)
    finally:
        lp.config.isotropic_matern_higher_order = saved
    assert desc[0]["family"] == [4, 4]
    return 2, desc


@pytest.mark.parametrize("name", ["product2d", "sum2d", "product3d", "radial2d", "product2d_factors"])
def test_matvec_on_resident_blocks_equals_the_host_vector_path(ctx, name):
    """`lpgp_kernel_matvec_dev` runs the kernels of `lpgp_kernel_matvec` with the same `splits`, on rows [v_off, v_off + n1) of V into
    rows [y_off, y_off + n0) of Y: with accumulate = 0 the rows are the host-vector product BIT FOR BIT, with accumulate = 1
    fl(old + product), and every other row of Y keeps its bits -- at row offsets that are no multiple of 64 and with 1, 4, 5 and 9
    right-hand sides (the pass loop's `+ r0 * ld`).  One descriptor per kernel variant.  The host-vector path itself is held once
    to `kernel_matrix @ V` summed in longdouble, within (ceil(n1 / 64) 16 + splits + 4) u |K| |V| per entry, doubled: the 16-deep
    chains of a wave per column tile, the four waves and the splits, and the entry's own few ulp between two kernels."""
    from linpde_gp_amd import _engine
    rng = np.random.default_rng(31)
    d, desc = _descriptor(name)
    X0, X1 = rng.uniform(-1, 1, (MV_N0, d)), rng.uniform(-1, 1, (MV_N1, d))
    P0, P1 = _engine.Points(ctx, X0), _engine.Points(ctx, X1)
    factors = name.endswith("_factors")
    if factors:
        ctx.set_option("asm_factors", 1)
    try:
        K = _engine.kernel_matrix(ctx, desc, P0, P1)
        for m in MV_COLUMNS:
            Vh, old = rng.standard_normal((MV_N, m)), rng.standard_normal((MV_N, m))
            V = _engine.DeviceVectors(ctx, MV_N, m, Vh)
            for v_off, y_off in MV_OFFSETS:
                want = _engine.kernel_matvec(ctx, desc, P0, P1, np.ascontiguousarray(Vh[v_off:v_off + MV_N1]))
                assert want.shape == (MV_N0, m) and np.isfinite(want).all() and np.all(np.any(want != 0.0, axis=0))
                rows = slice(y_off, y_off + MV_N0)
                keep = np.ones(MV_N, dtype=bool)
                keep[rows] = False
                for accumulate in (False, True):
                    Y = _engine.DeviceVectors(ctx, MV_N, m, old)
                    _engine.kernel_matvec_dev(ctx, desc, P0, P1, V, v_off, Y, y_off, accumulate)
                    got = Y.get()
                    what = (name, m, v_off, y_off, accumulate)
                    assert same_bits(got[rows], old[rows] + want if accumulate else want), what
                    assert same_bits(got[keep], old[keep]), what
                assert same_bits(V.get(), Vh)
            if m == MV_COLUMNS[-1]:
                tiles_r, tiles_c = -(-MV_N0 // 64), -(-MV_N1 // 64)
                splits = max(1, min(-(-4 * ctx.device_info()["cus"] // tiles_r), tiles_c))        # as `lpgp_kernel_matvec` does
                depth = tiles_c * 16 + splits + 4
                pr.longdouble_ok(MV_N1, depth)
                Vs = Vh[v_off:v_off + MV_N1]
                ref = K.astype(LD) @ Vs.astype(LD)
                ratio = pr.worst_ratio(want, ref, 2.0 * depth * pr.U * (np.abs(K) @ np.abs(Vs)))
                print(f"host-vector product {name}: error / bound {ratio:.3f} (splits {splits})")
                assert ratio <= 1.0, ratio
    finally:
        if factors:
            ctx.set_option("asm_factors", 0)
