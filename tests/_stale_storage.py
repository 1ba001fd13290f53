"""What the library's results may depend on when its device buffers come back dirty (tests/test_gpu_stale_storage.py,
tests/test_stale_storage_host.py).  The library never clears a buffer it hands out ("What a buffer holds"); the fill
mode of the device pool (`_hooks.pool_fill`) hands every buffer out poisoned, and a workload run under three fills must return the
same bits.  This module holds the layout predicates -- what of a matrix's padded storage the contract defines -- on plain NumPy
arrays, and the workloads: functions of the context that build everything from scratch and return named host arrays.  A plain
module the tests import, not a conftest."""
import gc
import types

import numpy as np

TILE = 128
FILLS = (0x00, 0xFF, 0x7F)          # zeros; every double a NaN; every double 1.38e306 (finite: gets through masks that swallow a NaN)


# ---- layout predicates (host only) ---------------------------------------------------------------------------------------
def padded(nb):
    return -(-nb // TILE) * TILE


def layout(blocks):
    """[(padded offset, rows, padded rows)] of the blocks of a matrix."""
    out, poff = [], 0
    for nb in blocks:
        out.append((poff, nb, padded(nb)))
        poff += padded(nb)
    return out


def defined_mask(pn, factored_rows):
    """The entries of a matrix's padded storage (pn x pn, [r, c]) that the contract defines: everything in the tiles below the tile
    diagonal; in a diagonal tile the lower triangle, and -- once the tile is factored (its rows < `factored_rows`) -- the strict
    upper triangle too, which the tile Cholesky stores as zeros.  Before the factorisation the strict upper triangle of a diagonal
    tile holds whatever the assembly's 64 x 64 tiles reached and stale storage elsewhere; tiles above the tile diagonal are never
    written.  Neither is read."""
    r = np.arange(pn)
    tr = r // TILE
    mask = tr[:, None] > tr[None, :]
    diag = tr[:, None] == tr[None, :]
    mask |= diag & (r[:, None] >= r[None, :])
    mask |= diag & (r[:, None] < factored_rows)
    return mask


def contract_violations(raw, blocks, factored_rows=0):
    """The padding contract on a read-out of `lpgp_test_mat_raw` (pn x pn, [r, c]): every padding row of every block holds exactly
    0.0 left of the diagonal and 1.0 on it; every padding column exactly 0.0 below the diagonal down to the padded size; a factored
    diagonal tile exactly 0.0 above its diagonal.  Returns the violations as strings (empty: the contract holds)."""
    pn = raw.shape[0]
    assert raw.shape == (pn, pn) and pn == sum(p for _, _, p in layout(blocks)), (raw.shape, blocks)
    bad = []
    for bi, (poff, n, p) in enumerate(layout(blocks)):
        for r in range(poff + n, poff + p):
            left, below = raw[r, :r], raw[r + 1:, r]
            if not np.all(left == 0.0):
                c = int(np.argmax(left != 0.0))
                bad.append(f"block {bi}: padding row {r} holds {raw[r, c]!r} at column {c}")
            if not raw[r, r] == 1.0:
                bad.append(f"block {bi}: padding row {r} holds {raw[r, r]!r} on the diagonal")
            if not np.all(below == 0.0):
                i = int(np.argmax(below != 0.0))
                bad.append(f"block {bi}: padding column {r} holds {raw[r + 1 + i, r]!r} at row {r + 1 + i}")
    for t in range(factored_rows // TILE):
        tile = raw[t * TILE:(t + 1) * TILE, t * TILE:(t + 1) * TILE]
        up = np.triu(tile, 1)
        if not np.all(up[np.triu_indices(TILE, 1)] == 0.0):
            bad.append(f"factored diagonal tile {t} is not zero above its diagonal")
    return bad


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- what a workload hands back ------------------------------------------------------------------------------------------
class Proof:
    """Proof of reuse: `filled` of the hook read around the allocations that matter.  matrix(make, cap) / rhs(make, pn, m) run
    `make` and record that at least one buffer and at least the bytes of the matrix (8 cap^2) or of the right-hand side were
    filled on its way."""

    def __init__(self, take):
        self.take, self.log = take, []

    def _around(self, kind, need, make):
        self.take()
        obj = make()
        count, nbytes = self.take()
        self.log.append((kind, need, count, nbytes))
        return obj

    def matrix(self, make, cap_rows):
        cap = padded(cap_rows)
        return self._around("matrix", 8 * cap * cap, make)

    def rhs(self, make, pn, m):
        return self._around("rhs", 8 * pn * padded(m + 1), make)

    def buffers(self, make, need):
        return self._around("buffers", need, make)


class Result:
    """out: every array the calls returned; raws: name -> (read-out of lpgp_test_mat_raw, blocks, factored padded rows);
    ref: whatever the reference check of the 0x00 run needs (host data only)."""

    def __init__(self):
        self.out, self.raws, self.ref = {}, {}, types.SimpleNamespace()

    def raw(self, ctx, name, mat, factored_rows):
        import _hooks
        self.raws[name] = (_hooks.mat_raw(ctx, mat).copy(), list(mat.block_sizes), int(factored_rows))


def _points(ctx, X):
    from linpde_gp_amd import _engine
    return _engine.Points(ctx, np.ascontiguousarray(X))


def _appender(ctx, pr, X, noise, capacity=None):
    from _backward import Appender
    return pr.matrix(lambda: Appender(ctx, X, noise, capacity), X.shape[0] if capacity is None else capacity)


def _rhs(ctx, pr, mat, m):
    from linpde_gp_amd import _engine
    return pr.rhs(lambda: _engine.Rhs(ctx, mat, m), mat.padded_n, m)


def _cross(ctx, pr, ap, Pt, m):
    K = _rhs(ctx, pr, ap.mat, m)
    for bi in range(ap.mat.num_blocks):
        K.cross_assemble(ap.kd, ap.pts[bi], Pt, bi)
    return K


def _case(res, tag, blocks, K0, V, L, r, kxx, mean, var):
    """The operands of one prediction as test_gpu_predict_backward.check_V / check_var / check_mean_z take them."""
    pn = sum(padded(nb) for nb in blocks)
    setattr(res.ref, tag, types.SimpleNamespace(blocks=list(blocks), n=sum(blocks), m=K0.shape[1], K0=K0, V=V, L=L, r=r, kxx=kxx, mean=mean,
                                                var=var, mat=types.SimpleNamespace(padded_n=pn)))


def _ride(ctx, pr, res, tag, ap, xt, r, m):
    """lpgp_potrf_predict at the m points `xt` from the blocks of `ap`; K0, V, L, mean, var into `res` under `tag`."""
    Pt = _points(ctx, xt)
    K = _cross(ctx, pr, ap, Pt, m)
    K0 = K.to_host()
    ap.mat.set_residual(r[:ap.mat.n])
    kxx = np.ones(m)
    mean, var = K.potrf_predict(None, kxx)
    assert ap.mat.check() == (0, -1)
    V, L = K.to_host(), ap.mat.todense("factor")
    res.out.update({tag + ".K0": K0, tag + ".V": V, tag + ".L": L, tag + ".mean": mean, tag + ".var": var})
    _case(res, tag.replace(".", "_"), ap.mat.block_sizes, K0, V, L, r[:ap.mat.n], kxx, mean, var)


def _predict(ctx, pr, res, tag, ap, xt, r, m):
    """lpgp_predict (mean and variance, the residual riding as the spare column) from the factored blocks in view."""
    Pt = _points(ctx, xt)
    K = _cross(ctx, pr, ap, Pt, m)
    K0 = K.to_host()
    ap.mat.set_residual(r[:ap.mat.n])
    kxx = np.ones(m)
    mean, var = K.predict(None, kxx)
    V, L = K.to_host(), ap.mat.todense("factor")
    res.out.update({tag + ".K0": K0, tag + ".V": V, tag + ".L": L, tag + ".mean": mean, tag + ".var": var})
    _case(res, tag.replace(".", "_"), ap.mat.block_sizes[:ap.mat.num_blocks], K0, V, L, r[:ap.mat.n], kxx, mean, var)
    return K


def observation_points(n):
    from test_gpu_predict_backward import observation_points as op
    return op(n)


# ---- a. rollback onto blocks of other sizes ------------------------------------------------------------------------------
A_FIRST, A_FAIL, A_AFTER = 129, 300, [1, 200, 128]          # padded 256 | 384 (rolled back) -> 128, 256, 128: tails of 127 and 56
A_N = A_FIRST + A_FAIL + 29                                 # rows on old factor rows, 128 has no tail at all
A_M = 3


def _a_inputs():
    X, noise = observation_points(A_N)
    rng = np.random.default_rng(11)
    return X, noise, rng.standard_normal(A_N), rng.uniform(0, 0.5, (A_M, 2))


def workload_a_appender(ctx, pr, real_failure):
    """[129, 300] factored; rolled back to one block -- a forced status and `truncate`, or (`real_failure`) a pivot of the second
    block broken, `lpgp_potrf` failing on it and `pop_block`, so that the storage holds the NaNs of the failed pivot --; then
    [1, 200, 128] appended on the old factor rows and `lpgp_potrf_predict` at m = 3."""
    import _hooks
    res = Result()
    X, noise, r, xt = _a_inputs()
    ap = _appender(ctx, pr, X, noise)
    ap.add(A_FIRST)
    assert ap.mat.potrf() == 0
    if real_failure:
        extra = np.zeros(A_FAIL)
        extra[5] = -10.0
        ap.add(A_FAIL, extra)
        assert ap.mat.potrf() == 256 + 5 + 1       # (what the failed block's rows hold now is undefined: not read)
        ap.drop(1)
    else:
        ap.add(A_FAIL)
        assert ap.mat.potrf() == 0
        res.raw(ctx, "first", ap.mat, 640)
        _hooks.force_status(ctx, ap.mat, 130)
        assert ap.mat.check()[0] == 130           # (padded row 129: the first padding row of block 0)
        ap.drop(1, truncate=True)
    assert (ap.mat.n, ap.mat.padded_n, ap.mat.num_blocks) == (A_FIRST, 256, 1)
    for nb in A_AFTER:
        ap.add(nb)
    res.raw(ctx, "appended", ap.mat, 256)
    _ride(ctx, pr, res, "ride", ap, xt, r, A_M)
    res.raw(ctx, "factored", ap.mat, ap.mat.padded_n)
    res.ref.X, res.ref.noise, res.ref.blocks = X, noise, [A_FIRST] + A_AFTER
    del ap
    gc.collect()
    return res


def workload_a_condition(ctx, pr, lazy, noise_kind, real_failure=False):
    """The same walk through `lpgp_mat_condition` (its padding and noise in ONE launch behind the assembly, finish_block_kernel):
    lazy 0 (factored in the call), 1 (enqueued) or 2 (assembled only); the noise a scalar, a vector or a dense block.
    `real_failure` (lazy 0 or 1, a noise vector or a dense block): the second block's noise breaks a pivot, so the factorisation really
    fails -- at lazy 0 the call itself drops the block, at lazy 1 `check` finds it and `truncate` drops it -- and the new padding goes
    on the NaNs of the failed pivot."""
    import _hooks
    from _backward import Appender
    from linpde_gp_amd import _engine
    res = Result()
    X, noise, r, xt = _a_inputs()
    ap = _appender(ctx, pr, X, noise)          # (for its matrix, descriptor and point list: the blocks go through condition)
    mat = ap.mat

    def condition(nb, broken=False):
        lo = mat.n
        P = _points(ctx, X[lo:lo + nb])
        row = [(ap.kd, Q) for Q in ap.pts] + [(ap.kd, None)]
        v = noise[lo:lo + nb].copy()
        if broken:
            v[5] = -10.0
        kw = {"scalar": {"noise_scalar": float(v[0])}, "vector": {"noise_diag": v}, "dense": {"noise_dense": np.diag(v)}}[noise_kind]
        info = mat.condition(nb, P, row, lazy=lazy, **kw)
        if broken and lazy == 0:
            assert info == 256 + 5 + 1                     # (the call has dropped the block again)
            return
        assert info == 0
        ap.pts.append(P)

    condition(A_FIRST)
    if real_failure:
        assert lazy in (0, 1) and noise_kind != "scalar"
        condition(A_FAIL, broken=True)
        if lazy == 1:
            assert mat.check() == (256 + 5 + 1, 1)
            ap.drop(1, truncate=True)
    else:
        condition(A_FAIL)
        _hooks.force_status(ctx, mat, 130)
        mat.check()
        ap.drop(1, truncate=True)
    assert (mat.n, mat.padded_n, mat.num_blocks) == (A_FIRST, 256, 1)
    for nb in A_AFTER:
        condition(nb)
    if lazy == 2:
        res.raw(ctx, "appended", mat, 0)
    _ride(ctx, pr, res, "ride", ap, xt, r, A_M)
    res.raw(ctx, "factored", mat, mat.padded_n)
    res.ref.X, res.ref.noise, res.ref.blocks = X, noise, [A_FIRST] + A_AFTER
    del ap, mat
    gc.collect()
    return res


# ---- b. growth -----------------------------------------------------------------------------------------------------------
B_BLOCKS, B_CLONE, B_MORE, B_M = [100, 77, 1, 513], 130, 5, 5
B_CAPS = [128, 256, 384, 1024]          # the capacity after each block: two geometric growths (x 1.5, rounded up to tiles), one exact


def workload_b(ctx, pr):
    """Capacity hint 128; [100, 77, 1, 513] appended and factored one by one (the copy and the cleared rows of mat_alloc go into
    poisoned storage); a clone of two blocks extended by [130] while the source goes on with [5]; predictions from both; a view
    of one block with a right-hand side of its own."""
    res = Result()
    n = sum(B_BLOCKS) + B_MORE
    X, noise = observation_points(n)
    rng = np.random.default_rng(12)
    r, xt = rng.standard_normal(n), rng.uniform(0, 0.5, (B_M, 2))
    ap = _appender(ctx, pr, X, noise, capacity=128)
    for k, nb in enumerate(B_BLOCKS):
        pr.matrix(lambda: ap.add(nb), B_CAPS[k]) if k else ap.add(nb)
        assert ap.mat.potrf() == 0
        res.raw(ctx, f"grown{k}", ap.mat, ap.mat.padded_n)
    from _backward import Appender
    ap2 = Appender.__new__(Appender)
    ap2.ctx, ap2.X, ap2.noise, ap2.kd = ctx, X, noise, ap.kd
    ap2.mat = pr.matrix(lambda: ap.mat.clone(2), 256)
    ap2.pts = list(ap.pts[:2])
    ap2.add(B_CLONE)
    ap.add(B_MORE)
    assert ap.mat.potrf() == 0
    _predict(ctx, pr, res, "source", ap, xt, r, B_M)
    _ride(ctx, pr, res, "clone", ap2, xt, r, B_M)
    res.raw(ctx, "source", ap.mat, ap.mat.padded_n)
    res.raw(ctx, "clone", ap2.mat, ap2.mat.padded_n)
    ap.mat.set_view(1)
    _predict(ctx, pr, res, "view", ap, xt, r, B_M)
    ap.mat.set_view(-1)
    res.ref.X, res.ref.noise, res.ref.blocks = X, noise, B_BLOCKS + [B_MORE]
    del ap, ap2
    gc.collect()
    return res


# ---- c. many ragged blocks -----------------------------------------------------------------------------------------------
C_CYCLE, C_MS = (1, 127, 129, 5), (1, 127, 128, 129)


def workload_c(ctx, pr, nblocks):
    """17 or 31 blocks of sizes cycling through (1, 127, 129, 5), every one ragged: `lpgp_rhs_create` clears their padding tails
    fifteen to a launch, so one full batch plus two tails, or two full batches plus one.  The cross-covariance through
    `lpgp_cross_assemble_row`; mean and variance, the mean alone from the weights, the variance alone; m on both sides of 128."""
    from linpde_gp_amd import _engine
    res = Result()
    blocks = [C_CYCLE[i % 4] for i in range(nblocks)]
    n = sum(blocks)
    X, noise = observation_points(n)
    rng = np.random.default_rng(13 + nblocks)
    r = rng.standard_normal(n)
    ap = _appender(ctx, pr, X, noise)
    for nb in blocks:
        ap.add(nb)
    assert ap.mat.potrf() == 0
    mat = ap.mat
    if nblocks <= 17:
        res.raw(ctx, "factored", mat, mat.padded_n)
    L = mat.todense("factor")
    res.out["L"] = L
    entries = [(ap.kd, P) for P in ap.pts]

    def cross(m, Pt):
        K = _rhs(ctx, pr, mat, m)
        K.cross_assemble_row(entries, Pt)
        return K

    Pts = {}
    for m in C_MS:                                      # no weights resident yet: the mean beside the variance is V^T z
        xt = np.random.default_rng(m).uniform(0, 0.5, (m, 2))
        xt[:min(m, 4)] = X[:min(m, 4)]                  # observation points: variance ~ 0
        Pt = Pts[m] = _points(ctx, xt)
        kxx = np.ones(m)
        K = cross(m, Pt)
        K0 = K.to_host()
        mat.set_residual(r)
        mean, var = K.predict(None, kxx)
        V = K.to_host()
        _, var_only = cross(m, Pt).predict(None, kxx, want_mean=False, want_var=True)
        res.out.update({f"m{m}.K0": K0, f"m{m}.V": V, f"m{m}.mean": mean, f"m{m}.var": var, f"m{m}.var_only": var_only})
        _case(res, f"m{m}", blocks, K0, V, L, r, kxx, mean, var)
        getattr(res.ref, f"m{m}").var_only = var_only
        del K
    res.out["w"] = mat.solve_weights(r)
    for m in C_MS:
        mean_w, _ = cross(m, Pts[m]).predict(None, None, want_mean=True, want_var=False)
        res.out[f"m{m}.mean_w"] = mean_w
        getattr(res.ref, f"m{m}").mean_w = mean_w
    res.ref.w, res.ref.X, res.ref.noise, res.ref.blocks = res.out["w"], X, noise, blocks
    del ap, mat
    gc.collect()
    return res


# ---- d. factorisation and substitution routes ----------------------------------------------------------------------------
def route_rows():
    """(id, kind, options, case, counters that must count / must not): one case each of the rows of
    test_gpu_predict_backward.ROWS that the storage contract is about, with the counters that row asserts."""
    import test_gpu_predict_backward as PB
    rows = {r[0]: r for r in PB.ROWS}
    pick = {"narrow": (PB.APP, 700), "fused_solve0_wide": (PB.APP, 127), "two_level": (PB.APP, 1100), "ride_default": (PB.APP, 700, 3),
            "ride_two_level": (PB.APP, 1100, 2), "ride_vchain": (PB.T12, 700, 0), "ride_back_to_back": (PB.T12, 700, 0),
            "ride_aug": (PB.APP, 1100, 3, "room")}
    out = []
    for name, case in pick.items():
        _, kind, opts, cases, must, must_not = rows[name]
        assert any(tuple(c) == tuple(case) for c in cases), (name, case)
        out.append((name, kind, opts, case, must, must_not))
    return out


def workload_d(ctx, pr, row):
    import test_gpu_predict_backward as PB
    from _backward import restored
    name, kind, opts, case, must, must_not = row
    res = Result()
    extra = 300 if name == "ride_aug" else 0           # test_augmented_ride_then_append's block behind the augmented ride
    with restored(ctx, PB.OPTIONS) as apply:
        apply(opts)
        blocks, m = case[0], case[1]
        pr.take()
        c = PB.Case(ctx, blocks, m, case[2] if len(case) > 2 else None, case[3] if len(case) > 3 else None, spare=extra).predict(kind)
        count, nbytes = pr.take()
        pn = c.mat.padded_n
        pr.log.append(("matrix+rhs", 8 * pn * pn + 8 * pn * padded(m + 1), count, nbytes))
        res.out.update({"K0": c.K0, "V": c.V, "L": c.L, "mean": c.mean, "var": c.var})
        res.raw(ctx, "factored", c.mat, pn)
        _case(res, "case", c.blocks, c.K0, c.V, c.L, c.r, c.kxx, c.mean, c.var)
        res.ref.case.routes = c.routes
        if extra:
            c.ap.add(extra)
            assert c.mat.potrf() == 0
            res.out["L_appended"] = c.mat.todense("factor")
            res.raw(ctx, "appended", c.mat, c.mat.padded_n)
            res.ref.X, res.ref.noise, res.ref.blocks = c.ap.X, c.ap.noise, list(blocks) + [extra]
        del c
        gc.collect()
    return res


CHAIN = {"resident": (512, {"chain_resident_max_rows": 64}), "two_kernel": (640, {"chain_resident_max_rows": 0, "chain_resident2_max_rows": 64}),
         "appended": (1300, {"chain_resident_max_rows": 64})}
CHAIN_OPTIONS = ("chain_resident_max_rows", "chain_resident2_max_rows", "chain_ahead", "chain_ahead_min_rows")


def workload_d_chain(ctx, pr, which):
    """The resident and the two-kernel panel chain at the smallest n of test_gpu_chain.py, and its appended-block case, through the
    package as there: factor, prediction, representer weights."""
    import linpde_gp_amd as lp
    from _backward import restored
    from test_gpu_chain import _posterior
    n, opts = CHAIN[which]
    res = Result()
    with restored(ctx, CHAIN_OPTIONS) as apply:
        apply(opts)
        prior, _, X, Y, b = _posterior(lp, n, seed=n)
        Xt = np.random.default_rng(1).uniform(-1, 1, (33, 2))
        cuts = [0, 130, 390, 1300] if which == "appended" else [0, n]
        pr.take()
        u = prior
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            u = u.condition_on_observations(Y[lo:hi], X[lo:hi], b=lp.randvars.Normal(np.zeros(hi - lo), 1e-3 * np.eye(hi - lo)))
        L = u.gram.cholesky()
        mean, var = u.predict(Xt)
        w = u.representer_weights
        count, nbytes = pr.take()
        pn = sum(padded(hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:]))
        pr.log.append(("matrix+rhs", 8 * pn * pn + 8 * pn * 128, count, nbytes))
        res.out.update({"L": np.asarray(L), "mean": np.asarray(mean), "var": np.asarray(var), "w": np.asarray(w)})
        res.ref.X, res.ref.Y, res.ref.Xt, res.ref.cuts = X, Y, Xt, cuts
        del u
        gc.collect()
    return res


# ---- e. solves -----------------------------------------------------------------------------------------------------------
E_BLOCKS = [300, 77, 1]


def workload_e(ctx, pr):
    """`lpgp_potrs` at 1 and 129 right-hand sides, `lpgp_solve_weights` by the resident kernel and by one launch per tile row."""
    from _backward import restored
    res = Result()
    n = sum(E_BLOCKS)
    X, noise = observation_points(n)
    rng = np.random.default_rng(14)
    B = rng.standard_normal((n, 129))
    ap = _appender(ctx, pr, X, noise)
    for nb in E_BLOCKS:
        ap.add(nb)
        assert ap.mat.potrf() == 0
    pn = ap.mat.padded_n
    res.out["potrs1"] = pr.buffers(lambda: ap.mat.potrs(B[:, 0]), 8 * pn)
    res.out["potrs129"] = pr.buffers(lambda: ap.mat.potrs(B), 8 * pn * 129)
    with restored(ctx, ("trsv_resident",)) as apply:
        for resident in (0, 1):
            apply({"trsv_resident": resident})
            res.out[f"weights{resident}"] = ap.mat.solve_weights(B[:, 1])
    res.raw(ctx, "factored", ap.mat, pn)
    res.ref.X, res.ref.noise, res.ref.blocks, res.ref.B = X, noise, E_BLOCKS, B
    del ap
    gc.collect()
    return res


# ---- g. the sampling chain -----------------------------------------------------------------------------------------------
G_BLOCKS, G_MS, G_DAMP = [200, 77], (127, 128, 129), 1e-3


def workload_g(ctx, pr):
    """`lpgp_trsm_lower`, `lpgp_rhs_inner`, `lpgp_rhs_matmul` (1 and 130 columns), then S = k(x, x) - V^T V by `lpgp_mat_sub_inner`,
    `add_diag`, `lpgp_potrf` and `lpgp_mat_factor_matmul`, at M = 127, 128, 129 points.  At M = 129 the right-hand side has been
    through `lpgp_predict` first, so its spare column holds L^{-1} r when `sub_inner` reads it.  `lpgp_gemm_host` at (37, 211, 130)."""
    from linpde_gp_amd import _engine
    res = Result()
    n = sum(G_BLOCKS)
    X, noise = observation_points(n)
    rng = np.random.default_rng(15)
    r = rng.standard_normal(n)
    ap = _appender(ctx, pr, X, noise)
    for nb in G_BLOCKS:
        ap.add(nb)
        assert ap.mat.potrf() == 0
    res.out["L"] = ap.mat.todense("factor")
    res.ref.cases = {}
    for M in G_MS:
        xt = np.random.default_rng(M).uniform(0, 0.5, (M, 2))
        Pt = _points(ctx, xt)
        V = _cross(ctx, pr, ap, Pt, M)
        K0 = V.to_host()
        if M == 129:
            ap.mat.set_residual(r)
            V.predict(None, np.ones(M))
        else:
            V.trsm_lower()
        Vh = V.to_host()
        inner = V.inner(V)
        Bs = {k: np.random.default_rng(M + k).standard_normal((M, k)) for k in (1, 130)}
        W = {k: pr.rhs(lambda: V.matmul(Bs[k]), ap.mat.padded_n, k).to_host() for k in (1, 130)}
        S = pr.matrix(lambda: _engine.GramMatrix(ctx, M), M)
        S.add_block(M)
        S.assemble(ap.kd, Pt, None, 0, 0)
        Kxx = S.todense("gram")
        S.sub_inner(0, V)
        Sub = S.todense("gram")
        S.add_diag(0, None, G_DAMP)
        res.raw(ctx, f"M{M}.schur", S, 0)
        assert S.potrf() == 0
        res.raw(ctx, f"M{M}.factored", S, S.padded_n)
        LS = S.todense("factor")
        Z = np.random.default_rng(M + 7).standard_normal((M, 5))
        shift = np.random.default_rng(M + 8).standard_normal(M)
        draws = S.factor_matmul(Z, shift)
        res.out.update({f"M{M}.K0": K0, f"M{M}.V": Vh, f"M{M}.inner": inner, f"M{M}.W1": W[1], f"M{M}.W130": W[130], f"M{M}.Kxx": Kxx,
                        f"M{M}.schur": Sub, f"M{M}.LS": LS, f"M{M}.draws": draws})
        res.ref.cases[M] = types.SimpleNamespace(K0=K0, V=Vh, inner=inner, W=W, B=Bs, Kxx=Kxx, schur=Sub, LS=LS, Z=Z, shift=shift, draws=draws)
        del V, S
    A, B = rng.standard_normal((37, 130)), rng.standard_normal((130, 211))
    res.out["gemm"] = pr.buffers(lambda: _engine.gemm(ctx, A, B), 8 * (37 * 130 + 130 * 211 + 37 * 211))
    res.ref.gemm = (A, B)
    res.ref.blocks, res.ref.L, res.ref.pn = G_BLOCKS, res.out["L"], ap.mat.padded_n
    del ap
    gc.collect()
    return res


# ---- f. inverse and evidence family --------------------------------------------------------------------------------------
F_BLOCKS = [200, 317]


def f_folds(n):
    """One fold of 140 rows (more than a tile: the large-fold path) and four of about 94 (the tile path); every row in a fold."""
    fold_of = np.empty(n, dtype=np.int32)
    fold_of[:140] = 0
    fold_of[140:] = 1 + np.arange(n - 140) % 4
    return fold_of, 5


def workload_f(ctx, pr):
    """`lpgp_mat_inverse`, `inverse_diag`, `evidence`, `loo`, `evidence_grad`, `evidence_grad_diag` and `cv` at their public launch
    shapes (the multi-trip shapes have their garbage tests in test_gpu_evidence_grad.py and test_gpu_trmm_chunks.py)."""
    from _backward import Appender, gram_points
    res = Result()
    n = sum(F_BLOCKS)
    X, noise = gram_points("m", n)
    rng = np.random.default_rng(16)
    r, y, v = rng.standard_normal(n), rng.standard_normal(n), rng.uniform(0.5, 2.0, F_BLOCKS[1])
    ap = _appender(ctx, pr, X, noise)
    for nb in F_BLOCKS:
        ap.add(nb)
        assert ap.mat.potrf() == 0
    mat, pn = ap.mat, ap.mat.padded_n
    dG = _appender(ctx, pr, X, 0.5 * noise)         # the derivative: an assembled, unfactored matrix of the same layout
    for nb in F_BLOCKS:
        dG.add(nb)
    ginv = pr.matrix(mat.inverse, pn)
    fold_of, nfolds = f_folds(n)
    out = res.out
    out["L"], out["dG"], out["inverse"] = mat.todense("factor"), dG.mat.todense("gram"), ginv.todense()
    out["inverse_diag"] = pr.buffers(mat.inverse_diag, 8 * pn)          # (at least the vector of the diagonal)
    out["evidence"] = np.array(mat.evidence(r))
    out["loo.mean"], out["loo.var"], out["loo.logp"], total = mat.loo(r, y)
    out["loo.total"] = np.array([total])
    out["grad"] = np.array(mat.evidence_grad(ginv, dG.mat, r))
    out["grad_diag"] = np.array(mat.evidence_grad_diag(ginv, 1, r, v, 0.3))
    mean, var, logp, total, covs = mat.cv(ginv, r, y, fold_of, nfolds, return_cov=True)
    out.update({"cv.mean": mean, "cv.var": var, "cv.logp": logp, "cv.total": np.array([total])})
    out.update({f"cv.cov{f}": c for f, c in enumerate(covs)})
    res.raw(ctx, "factored", mat, pn)
    res.ref.X, res.ref.noise, res.ref.blocks, res.ref.r, res.ref.y, res.ref.v, res.ref.scalar = X, noise, F_BLOCKS, r, y, v, 0.3
    del ap, dG, ginv, mat
    gc.collect()
    return res


# ---- h. the Kronecker assembly -------------------------------------------------------------------------------------------
H_GRIDS = {"13x11": ((13, 11), 0), "16x8_wide": ((16, 8), 1)}          # (slow, fast) extents, kron_wide: 1 forces the 16-byte stores
H_KERNEL = (1.7, [("matern", 2.5, 0.8), ("matern", 3.5, 1.1)])         # (an even fast extent: the wide kernel takes it)


def workload_h_grid(ctx, pr, which):
    """A block on a tensor grid through `lpgp_gram_assemble_grid` (every grid size: config.grid_assembly_min_points = 0), factored
    and predicted from, through the package as test_gpu_fused.py does."""
    import linpde_gp_amd as lp
    from linpde_gp_amd import config
    from _backward import restored
    (ns, nf), wide = H_GRIDS[which]
    res = Result()
    cf = lp.randprocs.covfuncs
    scale, ((_, nu0, l0), (_, nu1, l1)) = H_KERNEL
    prior = lp.GaussianProcess(lp.functions.Zero((2,)), scale * cf.TensorProduct(cf.Matern((), nu=nu0, lengthscales=l0), cf.Matern((), nu=nu1, lengthscales=l1)))
    f0, f1 = np.linspace(-1, 1, ns), np.linspace(-1, 1, nf)
    g = lp.domains.TensorProductGrid(f0, f1)
    XX = np.stack(np.meshgrid(f0, f1, indexing="ij"), axis=-1)
    Y = np.sin(3 * XX[..., 0]) * np.cos(2 * XX[..., 1])
    Xt = np.random.default_rng(ns).uniform(-1, 1, (7, 2))
    saved = config.grid_assembly_min_points
    with restored(ctx, ("kron_wide",)) as apply:
        apply({"kron_wide": wide})
        config.grid_assembly_min_points = 0
        try:
            pr.take()
            u = prior.condition_on_observations(Y, X=g, b=lp.randvars.Normal(np.zeros(Y.shape), 1e-2 * np.ones(ns * nf)))
            L = u.gram.cholesky()
            mean, var = u.predict(Xt)
            count, nbytes = pr.take()
            pn = padded(ns * nf)
            pr.log.append(("matrix+rhs", 8 * pn * pn + 8 * pn * 128, count, nbytes))
            res.out.update({"L": np.asarray(L), "mean": np.asarray(mean), "var": np.asarray(var)})
            res.raw(ctx, "factored", u._state.mat, pn)
            res.ref.X, res.ref.Y, res.ref.Xt = XX.reshape(-1, 2), Y.reshape(-1), Xt
            del u
            gc.collect()
        finally:
            config.grid_assembly_min_points = saved
    return res


# ---- h. the weighted and the mixed assembly ------------------------------------------------------------------------------
H_ROWS, H_M, H_DAMP = 130, 33, 1e-6         # one block of 130 rows (a tail of 126), 33 prediction points, noise H_DAMP x the largest diagonal entry


def workload_h_operator(ctx, pr, which):
    """One block of 130 rows assembled by `lpgp_gram_assemble_weighted` (the three-term variable-coefficient operator of
    test_gpu_varcoef.py on both sides: nine pairs) or by `lpgp_gram_assemble_mixed` (the ragged nine-slot stencil table of
    test_gpu_mixed.py over 300 points, -Laplacian on both sides), a scalar noise, factored, and predicted from through the
    matching cross assembly."""
    import linpde_gp_amd as lp
    from linpde_gp_amd import _engine
    res = Result()
    rng = np.random.default_rng(94)
    Xt = rng.uniform(-1, 1, (H_M, 2))
    Pt = _points(ctx, Xt)
    M = pr.matrix(lambda: _engine.GramMatrix(ctx, H_ROWS), H_ROWS)
    M.add_block(H_ROWS)
    if which == "weighted":
        import test_gpu_varcoef as VC
        from oracle import covfuncs as ocf
        X1 = rng.uniform(-1, 1, (H_ROWS, 2))
        P1 = _points(ctx, X1)
        W = VC.vr.weights(VC._OP3, X1)
        ident = [(None, ocf.identity(2))]
        M.assemble_weighted(VC._pairs(lp, VC._KERNEL2, VC._OP3, VC._OP3), W, None, P1, None, 0, 0)

        def cross(K):
            K.cross_assemble_weighted(VC._pairs(lp, VC._KERNEL2, VC._OP3, ident), W, P1, Pt, 0)
        res.ref.X1, res.ref.A1 = X1, None
    else:
        import test_gpu_mixed as MX
        X1 = rng.uniform(-1, 1, (300, 2))
        P1 = _points(ctx, X1)
        i1, w1 = MX._table(rng, H_ROWS, 9, 300)
        T1 = _engine.Mix(ctx, i1, w1, 300)
        kernel, D = MX._kernel(2), MX._lap(2)
        M.assemble_mixed(MX._desc(lp, kernel, D, D), P1, T1, None, None, 0, 0)

        def cross(K):
            K.cross_assemble_mixed(MX._desc(lp, kernel, D, {(0, 0): 1.0}), P1, T1, Pt, 0)
        res.ref.X1, res.ref.A1 = X1, MX.mr.dense_of(i1, w1, 300)
    G0 = M.todense("gram")
    damp = H_DAMP * float(np.max(np.diag(G0)))
    M.add_diag(0, None, damp)
    G = M.todense("gram")
    res.raw(ctx, "assembled", M, 0)
    assert M.potrf() == 0
    res.raw(ctx, "factored", M, M.padded_n)
    L = M.todense("factor")
    K = _rhs(ctx, pr, M, H_M)
    cross(K)
    K0 = K.to_host()
    r = np.random.default_rng(95).standard_normal(H_ROWS)
    M.set_residual(r)
    kxx = np.full(H_M, float(np.max(np.diag(G0))))
    mean, var = K.predict(None, kxx)
    V = K.to_host()
    res.out.update({"G0": G0, "G": G, "L": L, "K0": K0, "V": V, "mean": mean, "var": var})
    _case(res, "case", [H_ROWS], K0, V, L, r, kxx, mean, var)
    res.ref.Xt, res.ref.damp = Xt, damp
    del K, M
    gc.collect()
    return res


# ---- i. matrix-free ------------------------------------------------------------------------------------------------------
I_N, I_RANK = 300, 40


def workload_i_matvec(ctx, pr):
    """`lpgp_kernel_matvec` and `lpgp_kernel_matvec_dev` at the shapes of test_gpu_pcg_kernels.py (130 x 70 points, 1 and 9 right-hand
    sides, row offsets that are no multiple of 64, with and without accumulation)."""
    import test_gpu_pcg_kernels as PK
    from linpde_gp_amd import _engine
    res = Result()
    rng = np.random.default_rng(31)
    d, desc = PK._descriptor("sum2d")
    X0, X1 = rng.uniform(-1, 1, (PK.MV_N0, d)), rng.uniform(-1, 1, (PK.MV_N1, d))
    P0, P1 = _points(ctx, X0), _points(ctx, X1)
    res.out["K"] = _engine.kernel_matrix(ctx, desc, P0, P1)
    res.ref.V, res.ref.old = {}, {}
    for m in (1, 9):
        Vh, old = rng.standard_normal((PK.MV_N, m)), rng.standard_normal((PK.MV_N, m))
        res.ref.V[m], res.ref.old[m] = Vh, old
        V = pr.buffers(lambda: _engine.DeviceVectors(ctx, PK.MV_N, m, Vh), 8 * PK.MV_N * m)
        for v_off, y_off in PK.MV_OFFSETS:
            res.out[f"host.m{m}.v{v_off}"] = pr.buffers(
                lambda: _engine.kernel_matvec(ctx, desc, P0, P1, np.ascontiguousarray(Vh[v_off:v_off + PK.MV_N1])), 8 * PK.MV_N1 * m)
            for accumulate in (False, True):
                Y = _engine.DeviceVectors(ctx, PK.MV_N, m, old)
                _engine.kernel_matvec_dev(ctx, desc, P0, P1, V, v_off, Y, y_off, accumulate)
                res.out[f"dev.m{m}.v{v_off}.y{y_off}.acc{int(accumulate)}"] = Y.get()
                del Y
        del V
    gc.collect()
    return res


def workload_i_pivchol(ctx, pr):
    """One pivoted-Cholesky build of rank 40 at n = 300 on the device, by the walk of test_gpu_pivchol.py: every step is held to the
    device's own state there (row bit for bit, commit and diagonal at their running bounds, delta and S), under every fill."""
    import linpde_gp_amd as lp
    import _mfree_reference as mr
    import test_gpu_pivchol as PC
    res = Result()
    saved = lp.config.matrix_free
    lp.config.matrix_free = True
    try:
        G = PC.one_block(lp, I_N)
        pr.take()
        pc, fig = PC.walk(G, I_RANK, mr.PIVOT_RTOL)
        count, nbytes = pr.take()
        pr.log.append(("buffers", 8 * (I_RANK * I_N + 3 * I_N), count, nbytes))          # L and the work vector at least
        assert fig["stopped_by"] == "rank" and pc.rank == I_RANK
        res.out.update({"L": pc.to_host("L"), "d": pc.to_host("d"), "pivots": np.asarray(pc.pivots, dtype=np.int64), "delta": np.array([pc.delta])})
        res.ref.fig = fig
        del pc, G
        gc.collect()
    finally:
        lp.config.matrix_free = saved
    return res


def workload_i_pcg(ctx, pr, shape):
    """Three PCG steps at a shape of `_pcg_reference.STEP_SHAPES`, as test_each_step_against_the_reference_from_the_device_state drives
    them (the product applied on the host); the state after every step is returned, and the state before it for the reference.
    That test asserts no bit identity between runs, so pcg.hip was read first: its dots are two-stage sums without atomics and
    its header promises the same bits on every call.  The states are therefore compared bit for bit across the fills like every
    other result, and the 0x00 run is held to that test's own running bounds, step by step."""
    import _pcg_reference as ref
    from linpde_gp_amd import _engine
    import test_gpu_pcg_kernels as PK
    n, m, rank = shape
    res = Result()
    pb = ref.problem(n, m, rank)
    bn = ref.bnorm(pb.B)
    DV = _engine.DeviceVectors
    X, R, Z, P, Q = pr.buffers(lambda: [DV(ctx, n, m), DV(ctx, n, m, pb.B), DV(ctx, n, m), DV(ctx, n, m), DV(ctx, n, m)], 5 * 8 * n * m)
    it = pr.buffers(lambda: _engine.DevicePCG(ctx, n, m, pb.L, pb.S, pb.delta), 8 * rank * n)
    rel = it.start(R, Z, P, bn, PK.RTOL)
    res.out["start.rel"] = rel
    res.ref.before, res.ref.Q = [], []
    for k in range(ref.STEPS):
        state = (X.get(), R.get(), Z.get(), P.get())
        Qh = pb.matvec(state[3])
        Q.set(Qh)
        res.ref.before.append(state)
        res.ref.Q.append(Qh)
        rel = it.step(X, R, Z, P, Q, PK.RTOL)
        res.out.update({f"step{k}.X": X.get(), f"step{k}.R": R.get(), f"step{k}.Z": Z.get(), f"step{k}.P": P.get(), f"step{k}.rel": rel})
    res.ref.shape = shape
    del X, R, Z, P, Q, it
    gc.collect()
    return res
