"""The high-precision reference of the device-resident conjugate gradients (tests/_pcg_reference.py), checked on the CPU before the
device is held against it (tests/test_gpu_pcg_kernels.py):

* its `start` / `step` ARE `randprocs/_matrix_free.pcg`: ten iterations on a dense SPD matrix agree with the host loop;
* a plain float64 NumPy evaluation of one step lies inside the running error bounds (they are bounds of an evaluation with the
  device's summation depths; NumPy's pairwise sums and BLAS are no deeper);
* the bit-exact fma helper agrees with `a + s * b` wherever `s * b` is exact;
* the inputs of the device tests are well conditioned: sum|a b| / |sum a b| <= 100 for every column dot of the reference run at every
  shape the device tests use (a condition on the construction; the device tests assert the same cap on what they read back).
"""
import numpy as np
import pytest

import _pcg_reference as pr

LD = pr.LD


def test_ten_iterations_equal_the_host_loop():
    from linpde_gp_amd.randprocs import _matrix_free as mfree
    rng = np.random.default_rng(5)
    n, m, rank = 300, 5, 4
    G = rng.standard_normal((n, n))
    A = G @ G.T / n + np.eye(n)
    A = 0.5 * (A + A.T)
    B = rng.standard_normal((n, m))
    L = rng.standard_normal((rank, n)) / np.sqrt(n)
    C = rng.standard_normal((rank, rank))
    S = C @ C.T
    S *= 0.5 / np.linalg.eigvalsh(C.T @ (L @ L.T) @ C)[-1]
    pre = pr.Preconditioner(n, L, S, pr.DELTA)
    AL = A.astype(LD)
    st, _ = pr.start(pre, B, pr.bnorm(B), 0.0)
    for it in range(1, 11):
        st, _ = pr.step(pre, st, AL @ st.P, 0.0)
        X, info = mfree.pcg(lambda V: A @ V, B, pre, rtol=0.0, maxiter=it)
        assert info["iterations"] == it
        err = float(np.max(np.abs(X.astype(LD) - st.X)))
        assert err <= 1e-12 * float(np.max(np.abs(st.X))), (it, err)
        assert np.max(np.abs(info["rel_residual"] - st.rel.astype(np.double))) <= 1e-12 * float(np.max(st.rel))


@pytest.mark.parametrize("n,m,rank", [(63, 3, 2), (257, 4, 5), (300, 5, 0), (32769, 2, 3)])
def test_a_float64_step_lies_inside_the_bounds(n, m, rank):
    pb = pr.problem(n, m, rank)
    pre = pb.preconditioner()
    bn = pr.bnorm(pb.B)
    rtol = 1e-12
    # start
    Z = pre.solve(pb.B)
    st, bd = pr.start(pre, pb.B, bn, rtol)
    assert pr.worst_ratio(Z, st.Z, bd["Z"]) <= 1.0
    assert pr.worst_ratio(np.linalg.norm(pb.B, axis=0) / bn, st.rel, bd["rel"]) <= 1.0
    # one step of `_matrix_free.pcg`, statement by statement, from the float64 state (its rz is the float64 sum)
    X, R, P = np.zeros_like(pb.B), pb.B.copy(), Z.copy()
    rz = np.sum(R * Z, axis=0)
    for _ in range(2):
        Q = pb.matvec(P)
        st = pr.state(pre, X, R, Z, P, bn, rtol)
        new, bd = pr.step(pre, st, Q, rtol)
        pq = np.sum(P * Q, axis=0)
        alpha = rz / pq
        X = X + alpha * P
        R = R - alpha * Q
        Z = pre.solve(R)
        rz_new = np.sum(R * Z, axis=0)
        P = Z + (rz_new / rz) * P
        rz = rz_new
        ratios = {k: pr.worst_ratio(v, getattr(new, k), bd[k]) for k, v in (("X", X), ("R", R), ("Z", Z), ("P", P))}
        ratios["rel"] = pr.worst_ratio(np.linalg.norm(R, axis=0) / bn, new.rel, bd["rel"])
        print(f"float64 step n={n} m={m} rank={rank}: error / bound {ratios}")
        assert max(ratios.values()) <= 1.0, ratios
        # the bounds are bounds of ROUNDING: a step that is wrong in the last digits of alpha is far outside
        assert pr.worst_ratio(X + 1e-10 * alpha * P, new.X, bd["X"]) > 1.0


def test_the_preconditioner_uses_S_as_given():
    pb = pr.problem(257, 2, 5, symmetric=False)
    assert np.max(np.abs(pb.S - pb.S.T)) > 0.1 * np.max(np.abs(pb.S))
    pre = pb.preconditioner()
    Z = pre.apply(pb.B)
    want = (pb.B - pb.L.T @ (pb.S @ (pb.L @ pb.B))) / pb.delta
    assert pr.worst_ratio(want, Z, 2.0 * pre.bound(pb.B)) <= 1.0
    flipped = pr.Preconditioner(pb.n, pb.L, pb.S.T, pb.delta).apply(pb.B)
    assert pr.worst_ratio(flipped, Z, 2.0 * pre.bound(pb.B)) > 1e6          # a transposed S is seen


def test_exact_sums_and_the_fma_helper():
    rng = np.random.default_rng(3)
    # a dot that cancels to its last bits: exact against rational arithmetic
    from fractions import Fraction
    a = rng.standard_normal(200) * 2.0 ** rng.integers(-30, 30, 200)
    b = rng.standard_normal(200) * 2.0 ** rng.integers(-30, 30, 200)
    a, b = np.concatenate([a, -a]), np.concatenate([b, b * (1 + 2.0 ** -40)])
    want = sum(Fraction(x) * Fraction(y) for x, y in zip(a.tolist(), b.tolist()))
    got = pr.coldot(a[:, None], b[:, None])[0]
    hi = float(got)
    assert abs(Fraction(hi) + Fraction(float(got - LD(hi))) - want) <= Fraction(2) ** -63 * abs(want)
    # longdouble operands enter as two float64 parts each
    al, bl = a.astype(LD) * (1 + LD(2) ** -60), b.astype(LD) / 3
    fr = lambda v: [Fraction(float(x)) + Fraction(float(x - LD(float(x)))) for x in v]      # noqa: E731
    want = sum(x * y for x, y in zip(fr(al), fr(bl)))
    got = pr.coldot(al[:, None], bl[:, None])[0]
    assert abs(Fraction(float(got)) + Fraction(float(got - LD(float(got)))) - want) <= Fraction(2) ** -63 * abs(want)
    # fma: one rounding; equal to a + s * b wherever s * b is exact (s a power of two, or b with few bits)
    x, y = rng.standard_normal((65, 3)), rng.standard_normal((65, 3))
    for s in (1.0, -1.0, 0.5, -4.0, 2.0 ** -20):
        assert np.array_equal(pr.fma_exact(s, y, x), x + s * y)
    small = rng.integers(-1000, 1000, (65, 3)).astype(np.double)
    assert np.array_equal(pr.fma_exact(-3.0, small, x), x + -3.0 * small)
    # and NOT equal to the twice-rounded value in general: the helper is a real fma
    s = 1.0 + 2.0 ** -30
    z = pr.fma_exact(s, y, x)
    assert np.any(z != x + s * y)
    assert np.all(np.abs(z - (x.astype(LD) + LD(s) * y)) <= 0.5 * np.spacing(np.abs(z)))


@pytest.mark.parametrize("n,m,rank", [(63, 3, 2), (65, 5, 3), (255, 1, 1), (257, 4, 5), (32768, 2, 3), (32769, 2, 3), (40001, 5, 3),
                                      (100, 256, 2)])
def test_the_inputs_are_well_conditioned(n, m, rank):
    if (n, m) not in ((255, 1),):
        assert (n, m, rank) in pr.STEP_SHAPES
    pb = pr.problem(n, m, rank)
    pre = pb.preconditioner()
    st, _ = pr.start(pre, pb.B, pr.bnorm(pb.B), 1e-12)
    worst = max(float(np.max(v)) for v in st.cond.values())
    assert np.all(st.rz > 0)
    for _ in range(pr.STEPS):
        st, _ = pr.step(pre, st, pb.matvec(st.P), 1e-12)
        worst = max(worst, *(float(np.max(v)) for v in st.cond.values()))
        assert np.all(st.rz > 0) and np.all(st.active)
    print(f"n={n} m={m} rank={rank}: worst condition number of a column dot {worst:.2f}")
    assert worst <= pr.COND_MAX
