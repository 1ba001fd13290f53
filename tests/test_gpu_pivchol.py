"""The pivoted Cholesky of a Gram operator on the device (`csrc/pivchol.hip`, `lpgp_pivchol_*`), through the C ABI (the thin wrapper
`_engine.DevicePivotedCholesky`), one step at a time.

Every check is against the DEVICE'S OWN previous state, read back with `lpgp_pivchol_to_host`, so no conditioning-dependent
amplification enters a bound; reference and bounds are tests/_pivchol_reference.py (held on the CPU by test_pivchol_reference.py):
  pivot    == int(np.argmax(d_dev)) and value == d_dev[pivot], bit for bit (np.argmax takes the FIRST of equal entries; the operators
           here have a constant diagonal, so step 0 is a tie over all n entries, across every workgroup of the first stage, and
           duplicated points keep tying later); -1 exactly when a stop rule holds on the device's own numbers
  row      the row buffer == `lpgp_kernel_matrix(one point, X_j)[0]` bit for bit, block by block
  commit   |L[k, j] - ref| <= (k + 3) u (|g_j| + sum_t |L[t, p]| |L[t, j]|) / sqrt(d_p): the kernel's count is k fma + square root +
           division, + the noise add at j = p -- k + 2 off the pivot column, k + 3 on it; rows 0 .. k-1 untouched bit for bit
  diagonal |d_new[j] - max(d[j] - L_dev[k, j]^2, 0)| <= 2 u (d[j] + L_dev[k, j]^2); d_new[p] == 0.0; d_new >= 0
  finish   delta against max(longdouble mean of d_dev, floor d0) within (sum_depth(n) + 1) u mean|d| (sum_depth = ceil(n / 65 536) + 16:
           the per-thread chain of the first stage, two 256-wide trees; + 1 for the division) or u floor d0;
           S against longdouble delta I + L_dev L_dev^T within gram_depth(n) u |L||L|^T, gram_depth = ceil(n / 256) + 8 + 2
           (one workgroup per entry: per-thread fma chain, one 256-wide tree, and 2 for the shift on the diagonal, whose rounding
           u (|L_a|^2 + delta) is within 2 u |L_a|^2 because delta <= max d <= d[p_a] = L[a, p_a]^2 for every committed row -- the
           greedy pivot is the largest entry and d only falls; the floor 1e-8 d0 lies below every pivot the rtol rule lets through);
           S == S^T bit for bit.  Above 300 rows S is held against the reference on a sample of its rows (the first, the last, those
           around each multiple of 256) -- a 2 048 x 2 048 longdouble product takes minutes --, its symmetry everywhere
Sizes sit on the launch geometry: 256 threads per workgroup (255, 256, 257), one trip of the first argmax stage (65 536 rows: 65 537
takes a second trip), the commit kernel's LDS staging of L[t, p] in passes of 256 (max_rank 200 stays within one pass; 300 at n = 333
takes a second; rows 2 046 and 2 047 at n = 2 100 are the last the cap LPGP_PIVCHOL_MAX_RANK = 2 048 admits: eight passes, the last
entry of the LDS array; 17 and 65 are ragged against the unroll of 8).  Every test prints its worst error / bound ratios."""
import ctypes as C

import numpy as np
import pytest

import _mfree_reference as mr
import _pivchol_reference as pv

pytestmark = pytest.mark.gpu

LD, U = pv.LD, pv.U
FLOOR = mr.DELTA_FLOOR
LAP_BLOCKS = (70, 130, 1)


@pytest.fixture
def lp():
    import linpde_gp_amd
    saved = linpde_gp_amd.config.matrix_free
    linpde_gp_amd.config.matrix_free = True
    yield linpde_gp_amd
    linpde_gp_amd.config.matrix_free = saved


def same_bits(A, B):
    A, B = np.ascontiguousarray(A, dtype=np.double), np.ascontiguousarray(B, dtype=np.double)
    return A.shape == B.shape and np.array_equal(A.view(np.uint64), B.view(np.uint64))


def one_block(lp, n, noise=1e-2, kernel="matern52", duplicates=True):
    """n points in [-1, 1]^2 as one value block with a CONSTANT noise vector (the diagonal of G is constant: all n entries tie at step
    0); with `duplicates`, three of the points coincide, so their diagonal entries stay equal bit for bit at every step."""
    rng = np.random.default_rng([51, n])
    X = rng.uniform(-1.0, 1.0, (n, 2))
    if duplicates and n >= 8:
        X[n // 2] = X[1]
        X[n - 1] = X[1]
    u = mr.prior(lp, kernel).condition_on_observations(rng.standard_normal(n), X, b=lp.randvars.Normal(np.zeros(n), np.full(n, noise)))
    assert type(u).__name__ == "MatrixFreeConditionalGaussianProcess"
    return u._G


def three_blocks(lp):
    """The operator of test_gpu_mfree_solve.py: a value block with a noise VECTOR, a -Laplacian block with scalar noise, a value block
    of one point without noise."""
    from linpde_gp_amd.linfuncops import diffops
    rng = np.random.default_rng(23)
    n0, n1, n2 = LAP_BLOCKS
    X0, X1, X2 = rng.uniform(-1, 1, (n0, 2)), rng.uniform(-1, 1, (n1, 2)), np.array([[1.5, -1.5]])
    Y0, Y1, Y2 = rng.standard_normal(n0), rng.standard_normal(n1), rng.standard_normal(n2)
    u = mr.prior(lp, "matern52").condition_on_observations(Y0, X0, b=lp.randvars.Normal(np.zeros(n0), rng.uniform(1e-3, 1e-1, n0)))
    u = u.condition_on_observations(Y1, X1, L=-1.0 * diffops.Laplacian((2,)), b=lp.randvars.Normal(np.zeros(n1), 0.5))
    u = u.condition_on_observations(Y2, X2)
    assert u._G.device_ok() and [int(o) for o in u._G.offs] == [0, 70, 200, 201]
    return u._G


def locate(G, p):
    i = int(np.searchsorted(G.offs, p, side="right") - 1)
    return i, p - int(G.offs[i])


def noise_at(G, i, l):
    nz = G._noise[i]
    return 0.0 if nz is None else float(nz[l])


def eval_row(pc, G, p, descs=None):
    i, l = locate(G, p)
    for j, bj in enumerate(G.blocks):
        if G.sizes[j]:
            kd = G.desc(i, j) if descs is None else descs.setdefault((i, j), G.desc(i, j))
            pc.row(kd, G.blocks[i].points, l, bj.points, int(G.offs[j]))
    return i, l


def sample_rows(k):
    """all rows of S up to 300; beyond, the first, the last and those around every multiple of 256"""
    if k <= 300:
        return np.arange(k)
    rows = {0, 1, k - 2, k - 1}
    for b in range(256, k, 256):
        rows.update((b - 1, b, b + 1))
    return np.array(sorted(r for r in rows if 0 <= r < k))


def walk(G, max_rank, rtol, unchecked=0):
    """The whole loop with every check of the module docstring; the first `unchecked` steps are only driven (pivot, row, commit), to
    reach a late step at a cost the suite can carry.  Returns (pc, figures)."""
    from linpde_gp_amd import _engine
    ctx, n = G.ctx, G.n
    diag = G.diag()
    d0 = float(np.max(diag))
    pc = _engine.DevicePivotedCholesky(ctx, n, max_rank, diag, rtol)
    assert pc.d0 == d0 and pc.rank == 0 and same_bits(pc.to_host("d"), diag)
    fig = {"L": 0.0, "d": 0.0, "ties": 0, "stopped_by": None}
    room = min(max_rank, n)
    k = 0
    descs = {}
    while k < unchecked:
        p, value = pc.pivot()
        assert 0 <= p < n and value > rtol * d0, (k, p, value)
        i, l = eval_row(pc, G, p, descs)
        pc.commit(noise_at(G, i, l))
        k += 1
    assert pc.rank == k
    while True:
        d_dev = pc.to_host("d")
        p, value = pc.pivot()
        p_np = int(np.argmax(d_dev))
        assert same_bits(value, d_dev[p_np]), (k, value, d_dev[p_np])
        stop = k >= room or value <= rtol * d0
        assert (p == -1) == stop, (k, p, value, rtol * d0)
        if stop:
            fig["stopped_by"] = "rank" if k >= room else "rtol"
            break
        assert p == p_np, (k, p, p_np)
        fig["ties"] += int(np.sum(d_dev == d_dev[p_np]) > 1)
        # ---- the row
        i, l = eval_row(pc, G, p)
        row = pc.to_host("row")
        one = _engine.Points(ctx, G.blocks[i].X.reshape(G.sizes[i], -1)[l:l + 1])
        for j, bj in enumerate(G.blocks):
            if G.sizes[j]:
                want = _engine.kernel_matrix(ctx, G.desc(i, j), one, bj.points)[0]
                assert same_bits(row[G.offs[j]:G.offs[j + 1]], want), (k, i, j)
        # ---- the commit
        noise = noise_at(G, i, l)
        L_prev = pc.to_host("L")
        assert L_prev.shape == (k, n)
        pc.commit(noise)
        assert pc.rank == k + 1 and int(pc.pivots[-1]) == p
        L_now, d_new = pc.to_host("L"), pc.to_host("d")
        assert same_bits(L_now[:k], L_prev)
        g = row.astype(LD)
        g[p] += LD(noise)
        p_ref, L_ref, _ = pv.one_step(L_prev, d_dev, g)
        assert p_ref == p
        fig["L"] = max(fig["L"], pv.worst_ratio(L_now[k], L_ref, pv.commit_bound(L_prev, d_dev, np.abs(g).astype(np.double), p)))
        ref, bound = pv.diag_update(d_dev, L_now[k], p)
        fig["d"] = max(fig["d"], pv.worst_ratio(d_new, ref, bound))
        assert d_new[p] == 0.0 and not np.signbit(d_new[p]) and np.all(d_new >= 0.0)
        k += 1
    assert fig["L"] <= 1.0 and fig["d"] <= 1.0, fig
    # ---- finish
    d_dev, L_dev = pc.to_host("d"), pc.to_host("L")
    delta, S = pc.finish(FLOOR)
    assert pc.rank == k and S.shape == (k, k) and same_bits(pc.to_host("L"), L_dev) and same_bits(pc.to_host("d"), d_dev)
    mean_bound = (pv.sum_depth(n) + 1) * U * float(np.mean(np.abs(d_dev)))
    fig["delta"] = float(abs(LD(delta) - pv.delta_of(d_dev, d0, FLOOR))) / max(mean_bound, U * FLOOR * d0)
    assert delta >= FLOOR * d0 * (1 - U) and delta > 0.0
    if k:
        rows = sample_rows(k)
        Ll = L_dev.astype(LD)
        S_ref = LD(delta) * np.eye(k, dtype=LD)[rows] + Ll[rows] @ Ll.T
        fig["S"] = pv.worst_ratio(S[rows], S_ref, pv.gram_depth(n) * U * (np.abs(L_dev[rows]) @ np.abs(L_dev).T))
        assert np.array_equal(S, S.T)
    else:
        fig["S"] = 0.0
    assert fig["delta"] <= 1.0 and fig["S"] <= 1.0, fig
    assert len(set(pc.pivots.tolist())) == k
    return pc, fig


# (n, max_rank): n reached at (1, 17), (2, 17); max_rank 0, 1, 2, 17, 65, 200, and 300: a second LDS staging pass of the commit;
# one / two workgroups; 129 workgroups; a second argmax trip
SHAPES = [(1, 1), (1, 17), (2, 17), (255, 2), (256, 2), (257, 0), (257, 1), (257, 17), (333, 65), (333, 200), (333, 300), (32769, 3),
          (65537, 2)]


@pytest.mark.parametrize("n,max_rank", SHAPES)
def test_every_step_against_the_devices_own_state(lp, n, max_rank):
    G = one_block(lp, n)
    pc, fig = walk(G, max_rank, mr.PIVOT_RTOL)
    print(f"n = {n}, max_rank = {max_rank}: rank {pc.rank}, {fig['ties']} tied pivots; error / bound: L {fig['L']:.3f}, d {fig['d']:.3f}, "
          f"delta {fig['delta']:.3f}, S {fig['S']:.3f}")
    assert fig["stopped_by"] == "rank" and pc.rank == min(n, max_rank)          # (noise 1e-2: the rtol stop is out of reach)
    if pc.rank and n >= 2:
        assert fig["ties"] >= 1 and int(pc.pivots[0]) == 0                      # a constant diagonal: index 0 wins step 0


def test_the_last_rows_the_rank_cap_admits(lp):
    """max_rank = LPGP_PIVCHOL_MAX_RANK = 2 048 at n = 2 100: steps 0 .. 2 045 are only driven, steps 2 046 and 2 047 -- eight staging
    passes of 256, the last of them filling the LDS array to its last entry -- are held like every other, and so are delta and S."""
    from linpde_gp_amd import _lib
    cap = _lib.PIVCHOL_MAX_RANK
    assert cap == 2048
    G = one_block(lp, 2100)
    pc, fig = walk(G, cap, mr.PIVOT_RTOL, unchecked=cap - 2)
    print(f"n = 2100, max_rank = {cap}: rank {pc.rank}; error / bound at steps {cap - 2}, {cap - 1}: L {fig['L']:.2e}, d {fig['d']:.3f}; "
          f"delta {fig['delta']:.3f}, S (sampled rows) {fig['S']:.3f}")
    assert fig["stopped_by"] == "rank" and pc.rank == cap


@pytest.mark.parametrize("max_rank", [17, 200])
def test_three_blocks_with_a_laplacian_and_a_noise_vector(lp, max_rank):
    G = three_blocks(lp)
    pc, fig = walk(G, max_rank, mr.PIVOT_RTOL)
    in_block = np.bincount(np.searchsorted(G.offs, pc.pivots, side="right") - 1, minlength=3)
    print(f"three blocks, max_rank = {max_rank}: rank {pc.rank}, pivots per block {in_block.tolist()}; error / bound: L {fig['L']:.3f}, "
          f"d {fig['d']:.3f}, delta {fig['delta']:.3f}, S {fig['S']:.3f}")
    assert (pc.rank == max_rank or fig["stopped_by"] == "rtol") and pc.rank >= 17
    assert int(np.searchsorted(G.offs, pc.pivots[0], side="right") - 1) == 1    # the Laplacian block has the largest diagonal


def test_the_rtol_stop(lp):
    """ExpQuad with noise 1e-6: the remaining diagonal falls below 1e-2 d0 long before 65 pivots.  `walk` asserts at every step that the
    pivot is -1 exactly when value <= rtol d0 on the device's own numbers; here that rule must be the one that ends the loop."""
    G = one_block(lp, 255, noise=1e-6, kernel="expquad")
    pc, fig = walk(G, 65, 1e-2)
    print(f"rtol stop: rank {pc.rank} of 65; error / bound: L {fig['L']:.3f}, d {fig['d']:.3f}, delta {fig['delta']:.3f}, S {fig['S']:.3f}")
    assert fig["stopped_by"] == "rtol" and 0 < pc.rank < 65


def test_two_builds_give_the_same_bits(lp):
    G = one_block(lp, 333)
    out = []
    for _ in range(2):
        pc, _fig = walk(G, 17, mr.PIVOT_RTOL)
        out.append((pc.to_host("L"), pc.to_host("d"), pc.pivots, pc.delta))
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2]) and out[0][3] == out[1][3]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def snapshot(pc):
    return pc.to_host("L"), pc.to_host("d"), pc.to_host("row"), pc.rank, pc.pivots.tolist()


def unchanged(pc, snap):
    now = snapshot(pc)
    return same_bits(now[0], snap[0]) and same_bits(now[1], snap[1]) and same_bits(now[2], snap[2]) and now[3:] == snap[3:]


def test_refusals_leave_the_object_untouched(lp):
    from linpde_gp_amd import _engine, _lib
    G = three_blocks(lp)
    ctx, n = G.ctx, G.n
    P = [b.points for b in G.blocks]
    pc = _engine.DevicePivotedCholesky(ctx, n, 17, G.diag(), mr.PIVOT_RTOL)
    refused = lambda match: pytest.raises(_lib.LpgpError, match=match)      # noqa: E731
    # nothing pending yet
    snap = snapshot(pc)
    with refused("lpgp_pivchol_commit: no pivot pending"):
        pc.commit(0.0)
    with refused("lpgp_pivchol_row: no pivot pending"):
        pc.row(G.desc(0, 0), P[0], 0, P[0], 0)
    assert unchanged(pc, snap)
    # one full step, so that L, d and the row buffer hold something
    p, _ = pc.pivot()
    eval_row(pc, G, p)
    i, l = locate(G, p)
    pc.commit(noise_at(G, i, l))
    p, _ = pc.pivot()
    i, l = locate(G, p)
    snap = snapshot(pc)
    with refused("lpgp_pivchol_commit: the row pieces do not tile"):          # no piece at all
        pc.commit(0.0)
    assert unchanged(pc, snap)
    pc.row(G.desc(i, 0), P[i], l, P[0], 0)
    snap = snapshot(pc)
    with refused("overlap"):                                                   # the same piece again
        pc.row(G.desc(i, 0), P[i], l, P[0], 0)
    with refused("overlap"):                                                   # 130 columns from 69 on: one column into the first piece
        pc.row(G.desc(i, 1), P[i], l, P[1], 69)
    for off in (-1, 72, n, n + 5, 2 ** 62):                                    # 130 columns that leave [0, 201)
        with refused("leave"):
            pc.row(G.desc(i, 1), P[i], l, P[1], off)
    with refused("lpgp_pivchol_row: point"):
        pc.row(G.desc(i, 1), P[i], G.sizes[i], P[1], 70)
    with refused("lpgp_pivchol_row: point"):
        pc.row(G.desc(i, 1), P[i], -1, P[1], 70)
    with refused("lpgp_pivchol_row: dimension mismatch"):
        pc.row(G.desc(i, 1), P[i], l, _engine.Points(ctx, np.zeros((130, 1))), 70)
    with refused("lpgp_pivchol_row: dimension mismatch"):
        pc.row(G.desc(i, 1), _engine.Points(ctx, np.zeros((G.sizes[i], 3))), l, P[1], 70)
    with refused("lpgp_pivchol_commit: the row pieces do not tile"):          # a gap: blocks 1 and 2 missing
        pc.commit(0.0)
    assert unchanged(pc, snap)                                                 # (every refusal since the first piece: row buffer included)
    pc.row(G.desc(i, 2), P[i], l, P[2], 200)
    snap = snapshot(pc)
    with refused("lpgp_pivchol_commit: the row pieces do not tile"):          # a gap in the middle
        pc.commit(0.0)
    assert unchanged(pc, snap)
    # the loop goes on from where it stood: pivot again (the same one), the whole row, commit
    p2, _ = pc.pivot()
    assert p2 == p
    eval_row(pc, G, p)
    pc.commit(noise_at(G, i, l))
    assert pc.rank == 2
    # a borrowed factor cannot be destroyed; a handle that is not finished cannot be borrowed
    with refused("lpgp_pcg_create_pivchol"):
        _engine.DevicePCG.from_resident(pc, 3, np.eye(2))
    delta, S = pc.finish(FLOOR)
    snap = snapshot(pc)
    with refused("lpgp_pivchol_pivot: the factorisation is finished"):
        pc.pivot()
    with refused("lpgp_pivchol_row: the factorisation is finished"):
        pc.row(G.desc(0, 0), P[0], 0, P[0], 0)
    with refused("lpgp_pivchol_commit: the factorisation is finished"):
        pc.commit(0.0)
    with refused("lpgp_pivchol_finish: the factorisation is finished"):
        pc.finish(FLOOR)
    with refused("lpgp_pivchol_to_host"):
        _lib.check(_lib.lib.lpgp_pivchol_to_host(ctx._h, pc._h, 3, _lib.as_pd(np.empty(n))), "lpgp_pivchol_to_host")
    assert unchanged(pc, snap)
    it = _engine.DevicePCG.from_resident(pc, 3, np.linalg.inv(S))
    assert _lib.lib.lpgp_pivchol_destroy(pc._h) != 0 and b"borrow" in _lib.lib.lpgp_last_error()
    assert unchanged(pc, snap)
    del it
    # create
    with refused("lpgp_pivchol_create: rank"):
        _engine.DevicePivotedCholesky(ctx, 5000, 2049, np.ones(5000), 1e-6)
    with refused("lpgp_pivchol_create"):
        _lib.check(_lib.lib.lpgp_pivchol_create(ctx._h, 0, 1, _lib.as_pd(np.ones(1)), 1e-6, C.byref(C.c_void_p())), "lpgp_pivchol_create")
    # a NaN in the diagonal is an error, not a pivot
    bad = np.ones(300)
    bad[290] = np.nan
    pn = _engine.DevicePivotedCholesky(ctx, 300, 3, bad, 1e-6)
    with refused("NaN"):
        pn.pivot()
    with refused("NaN"):
        pn.finish(FLOOR)
    assert pn.rank == 0


def test_refused_inside_a_multi_gpu_job_and_on_another_context(lp):
    """A second context on the same device: a handle of the first is refused there; once it has joined a job of one rank over the
    host-staged transport it is distributed, and every entry point refuses it before it looks at anything else."""
    from linpde_gp_amd import _engine, _lib
    G = one_block(lp, 64)
    ctx = G.ctx
    pc = _engine.DevicePivotedCholesky(ctx, 64, 3, G.diag(), 1e-6)
    ctx2 = _engine.Context(ctx.device)
    try:
        with pytest.raises(_lib.LpgpError, match="another context"):
            _lib.check(_lib.lib.lpgp_pivchol_pivot(ctx2._h, pc._h, C.byref(C.c_int64()), C.byref(C.c_double())), "lpgp_pivchol_pivot")
        pc2 = _engine.DevicePivotedCholesky(ctx2, 64, 3, G.diag(), 1e-6)
        pts = _engine.Points(ctx2, np.zeros((64, 2)))
        exchange = _lib.HOST_EXCHANGE_FN(lambda user, op, buf, nbytes, root: 0)
        _lib.check(_lib.lib.lpgp_dist_init_host(ctx2._h, 0, 1, exchange, None), "lpgp_dist_init_host")
        for call in (lambda: pc2.pivot(), lambda: pc2.row(G.desc(0, 0), pts, 0, pts, 0), lambda: pc2.commit(0.0), lambda: pc2.finish(FLOOR),
                     lambda: pc2.to_host("d"), lambda: _engine.DevicePivotedCholesky(ctx2, 64, 3, G.diag(), 1e-6),
                     lambda: _engine.DevicePCG.from_resident(pc2, 1, None)):
            with pytest.raises(_lib.LpgpError, match="single GPU only"):
                call()
        assert pc2.rank == 0
        del pc2, pts
    finally:
        ctx2.close()
    p, v = pc.pivot()
    assert p == 0 and v == G.diag()[0]
