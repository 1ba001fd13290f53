"""Every result is independent of stale device storage.  The library never clears a buffer it hands out: the pool gives cached
buffers out again with whatever their last owner left in them, the persistent scratch is kept across calls, a matrix's own storage
is reused in place after a rollback.  What makes that safe is the storage contract ("What a buffer holds"): padding rows
and columns are cleared exactly where they are read, everything else is written before it is read.  Here every workload of
tests/_stale_storage.py runs with the pool's fill mode on (`lpgp_test_pool_fill`: every buffer handed out is first filled, on the
panel stream) under three fills -- 0x00, 0xFF (every double a NaN) and 0x7F (every double 1.38e306, finite) -- and

  results   every returned array is bit-identical across the fills (`tobytes()`: NaN payloads would count) and finite: these paths
            promise run-to-run bit identity, so a difference is a read of storage nobody wrote (or a fill on the panel stream that
            overtook a first use on another stream);
  raw       read-outs of the matrix storage are bit-identical where the contract defines them (`_stale_storage.defined_mask`), every
            padding row holds exactly 0.0 left of the diagonal and 1.0 on it, every padding column 0.0 below it, a factored diagonal
            tile 0.0 above its diagonal (`contract_violations`); tiles above the tile diagonal are not compared;
  reference the 0x00 run alone is held to the long-double checks and bars of tests/_backward.py and
            tests/test_gpu_predict_backward.py, and to those of the test file a workload is taken from (evidence, cv, chain, fused,
            varcoef, mixed, pcg, pivchol: imported, none invented here), so that "identical" cannot mean "identically wrong";
  reuse     `filled` of the hook proves that the workload took poisoned buffers: around the allocation of a matrix at least its
            8 cap^2 bytes, around a right-hand side at least its size.

One test per workload and fill; the 0x00 run of a workload is computed once and shared by the other two."""
import gc
import types

import numpy as np
import pytest
import scipy.linalg

import _hooks
import _stale_storage as S
from _backward import EPS, LD, Appender, backward_error, mtv, mv, solve_backward_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


WORKLOADS = {
    "a_truncate": lambda ctx, pr: S.workload_a_appender(ctx, pr, False),
    "a_failed_potrf_pop": lambda ctx, pr: S.workload_a_appender(ctx, pr, True),
    "a_condition_failed_lazy0_vector": lambda ctx, pr: S.workload_a_condition(ctx, pr, 0, "vector", True),
    "a_condition_failed_lazy1_dense": lambda ctx, pr: S.workload_a_condition(ctx, pr, 1, "dense", True),
    "b_growth": S.workload_b,
    "c_ragged17": lambda ctx, pr: S.workload_c(ctx, pr, 17),
    "c_ragged31": lambda ctx, pr: S.workload_c(ctx, pr, 31),
    "e_solves": S.workload_e,
    "f_evidence": S.workload_f,
    "g_sampling": S.workload_g,
}
for _lazy in (0, 1, 2):                 # the full cross: the padding launch differs with the laziness and with the kind of noise
    for _kind in ("scalar", "vector", "dense"):
        WORKLOADS[f"a_condition_lazy{_lazy}_{_kind}"] = (lambda lazy, kind: lambda ctx, pr: S.workload_a_condition(ctx, pr, lazy, kind))(_lazy, _kind)
for _which in ("weighted", "mixed"):
    WORKLOADS["h_" + _which] = (lambda which: lambda ctx, pr: S.workload_h_operator(ctx, pr, which))(_which)
I_PCG_SHAPES = [(257, 4, 5), (32769, 2, 3), (100, 256, 2)]       # of _pcg_reference.STEP_SHAPES: one block, the dots' second trip, all 256 columns
WORKLOADS["i_matvec"] = S.workload_i_matvec
WORKLOADS["i_pivchol"] = S.workload_i_pivchol
for _shape in I_PCG_SHAPES:
    WORKLOADS["i_pcg_%dx%d_rank%d" % _shape] = (lambda shape: lambda ctx, pr: S.workload_i_pcg(ctx, pr, shape))(_shape)
for _which in S.H_GRIDS:
    WORKLOADS["h_grid_" + _which] = (lambda which: lambda ctx, pr: S.workload_h_grid(ctx, pr, which))(_which)
for _row in S.route_rows():
    WORKLOADS["d_" + _row[0]] = (lambda row: lambda ctx, pr: S.workload_d(ctx, pr, row))(_row)
for _which in S.CHAIN:
    WORKLOADS["d_chain_" + _which] = (lambda which: lambda ctx, pr: S.workload_d_chain(ctx, pr, which))(_which)
WORKLOADS = dict(sorted(WORKLOADS.items()))

_base = {}


def run(ctx, name, fill):
    with _hooks.pool_fill(ctx, fill) as take:
        pr = S.Proof(take)
        res = WORKLOADS[name](ctx, pr)
        ctx.sync()
        gc.collect()
    res.log = pr.log
    return res


# ---- the reference checks of the 0x00 run --------------------------------------------------------------------------------
def gram(ctx, X, noise, blocks):
    """The Gram matrix of the blocks as the device assembles it: a twin that is never factored."""
    twin = Appender(ctx, X, noise)
    for nb in blocks:
        twin.add(nb)
    return twin.mat.todense("gram")


def check_factor(G, L, tag):
    import test_gpu_predict_backward as PB
    be, be_ref = backward_error(G, L), backward_error(G, np.linalg.cholesky(G))
    print(f"\n[{tag}] factor backward error {be:.3e} (LAPACK {be_ref:.3e})")
    assert be <= PB.RATIO_FACTOR * be_ref and be <= PB.CEIL_FACTOR * G.shape[0] * EPS, f"{tag}: factor backward error {be:.3e}, LAPACK's {be_ref:.3e}"


def check_prediction(c, tag):
    import test_gpu_predict_backward as PB
    PB.check_V(c, tag)
    PB.check_var(c, tag)
    PB.check_mean_z(c, tag)


def reference_a(ctx, name, res):
    check_prediction(res.ref.ride, name)
    check_factor(gram(ctx, res.ref.X, res.ref.noise, res.ref.blocks), res.ref.ride.L, name)


def reference_b(ctx, name, res):
    for tag in ("source", "clone", "view"):
        check_prediction(getattr(res.ref, tag), f"{name} {tag}")
    check_factor(gram(ctx, res.ref.X, res.ref.noise, res.ref.blocks), res.ref.source.L, name)


def reference_c(ctx, name, res):
    import test_gpu_predict_backward as PB
    G = gram(ctx, res.ref.X, res.ref.noise, res.ref.blocks)
    check_factor(G, res.out["L"], name)
    for m in S.C_MS:
        c = getattr(res.ref, f"m{m}")
        check_prediction(c, f"{name} m={m}")
        # the variance alone (col_reduce_kernel: another order of the last four partial sums than col_reduce2_kernel's) at the same
        # bound; the mean from the weights is K0^T w at the bound of col_reduce_kernel's sum
        alone = types.SimpleNamespace(**vars(c))
        alone.var = c.var_only
        PB.check_var(alone, f"{name} m={m} variance alone")
        ref = mtv(c.K0, res.ref.w.astype(LD)[:, None])[:, 0]
        err = np.abs(c.mean_w.astype(LD) - ref).astype(np.float64)
        bound = PB.sum_bound(c.mat.padded_n) * (np.abs(c.K0).T @ np.abs(res.ref.w))
        assert np.all(err <= bound), f"{name} m={m}: K0^T w: worst {np.max(err / bound):.2f} of the bound"
    r = getattr(res.ref, f"m{S.C_MS[0]}").r
    be = solve_backward_error(G, res.ref.w, r)
    be_ref = solve_backward_error(G, scipy.linalg.cho_solve((np.linalg.cholesky(G), True), r), r)
    assert be <= PB.RATIO_SOLVE * be_ref, f"{name}: solve_weights backward error {be:.3e}, cho_solve's {be_ref:.3e}"


def reference_d(ctx, name, res):
    import test_gpu_predict_backward as PB
    c = res.ref.case
    row = next(r for r in S.route_rows() if "d_" + r[0] == name)
    PB.check_case(c, name, row[4], row[5])
    if "L_appended" in res.out:
        check_factor(gram(ctx, res.ref.X, res.ref.noise, res.ref.blocks), res.out["L_appended"], name + " appended")


def reference_d_chain(ctx, name, res):
    """The bars of test_gpu_chain.py: the oracle's posterior to 1e-8, L L^T against its Gram matrix to 4e-12."""
    from oracle import covfuncs as ocf
    from oracle import gp as ogp
    okern = [(1.69, [("matern", 2.5, 0.35), ("matern", 1.5, 0.35)])]
    X, Y, Xt, cuts = res.ref.X, res.ref.Y, res.ref.Xt, res.ref.cuts
    post = ogp.condition(okern, [ogp.ObsBlock(X[lo:hi], ocf.identity(2), Y[lo:hi], 0.0, 1e-3) for lo, hi in zip(cuts[:-1], cuts[1:])])
    m, v, L = res.out["mean"], res.out["var"], res.out["L"]
    assert np.max(np.abs(m - post.mean(Xt))) <= 1e-8 * np.max(np.abs(post.mean(Xt)))
    assert np.max(np.abs(v - post.var(Xt))) <= 1e-8 * np.max(np.abs(post.var(Xt)))
    if len(cuts) == 2:
        np.testing.assert_allclose(L @ L.T, post.G, rtol=0, atol=1e-12 * np.max(np.abs(post.G)) * 4)


def reference_e(ctx, name, res):
    """potrs at the bar of test_gpu_potrf_backward.check_solves (8 x cho_solve's normwise backward error), solve_weights at
    test_gpu_predict_backward's (2 x)."""
    import test_gpu_potrf_backward as FB
    import test_gpu_predict_backward as PB
    G = gram(ctx, res.ref.X, res.ref.noise, res.ref.blocks)
    Lref, B = np.linalg.cholesky(G), res.ref.B
    for key, b, ratio in (("potrs1", B[:, :1], FB.RATIO_SOLVE), ("potrs129", B, FB.RATIO_SOLVE), ("weights0", B[:, 1:2], PB.RATIO_SOLVE),
                          ("weights1", B[:, 1:2], PB.RATIO_SOLVE)):
        be = solve_backward_error(G, res.out[key], b)
        be_ref = solve_backward_error(G, scipy.linalg.cho_solve((Lref, True), b), b)
        print(f"\n[{name} {key}] backward error {be:.3e} (cho_solve {be_ref:.3e})")
        assert be <= ratio * be_ref, f"{name} {key}: backward error {be:.3e}, cho_solve's {be_ref:.3e}"


def gamma(k):
    return k * EPS / (1 - k * EPS)


def reference_g(ctx, name, res):
    """`trsm_lower` / `predict` at the bar of the substitution; inner, matmul, sub_inner, factor_matmul and gemm against long-double
    products of the device's own operands at the a-priori bound gamma_k of a sum of k products (test_gpu_predict_backward.
    test_trsm_lower_inner_matmul states them so), the Schur complement's factor at the bars of a factor."""
    import types
    import test_gpu_predict_backward as PB
    pn = res.ref.pn
    for M, c in res.ref.cases.items():
        tag = f"{name} M={M}"
        PB.check_V(types.SimpleNamespace(K0=c.K0, V=c.V, L=res.ref.L, blocks=res.ref.blocks), tag)
        VtV = np.abs(c.V).T @ np.abs(c.V)
        err = np.abs(c.inner.astype(LD) - mtv(c.V, c.V.astype(LD))).astype(np.float64)
        assert np.all(err <= gamma(pn) * VtV), f"{tag} inner: worst {np.max(err / (gamma(pn) * VtV)):.2f} of the bound"
        for k in (1, 130):
            err = np.abs(c.W[k].astype(LD) - mv(c.V, c.B[k].astype(LD))).astype(np.float64)
            bound = gamma(S.padded(M + 1)) * (np.abs(c.V) @ np.abs(c.B[k]))
            assert np.all(err <= bound), f"{tag} matmul {k}: worst {np.max(err / bound):.2f} of the bound"
        err = np.abs(c.schur.astype(LD) - (c.Kxx.astype(LD) - mtv(c.V, c.V.astype(LD)))).astype(np.float64)
        bound = gamma(pn + 1) * (VtV + np.abs(c.Kxx))
        low = np.tril(np.ones((M, M), dtype=bool))
        assert np.all(err[low] <= bound[low]), f"{tag} sub_inner: worst {np.max(err[low] / bound[low]):.2f} of the bound"
        A = np.tril(c.schur) + np.tril(c.schur, -1).T + S.G_DAMP * np.eye(M)
        check_factor(A, c.LS, tag + " Schur complement")
        err = np.abs(c.draws.astype(LD) - (c.shift.astype(LD)[:, None] + mv(c.LS, c.Z.astype(LD)))).astype(np.float64)
        bound = gamma(M + 1) * (np.abs(c.LS) @ np.abs(c.Z) + np.abs(c.shift)[:, None])
        assert np.all(err <= bound), f"{tag} factor_matmul: worst {np.max(err / bound):.2f} of the bound"
    A, B = res.ref.gemm
    err = np.abs(res.out["gemm"].astype(LD) - mv(A, B.astype(LD))).astype(np.float64)
    bound = gamma(130) * (np.abs(A) @ np.abs(B))
    assert np.all(err <= bound), f"{name} gemm: worst {np.max(err / bound):.2f} of the bound"


def reference_f(ctx, name, res):
    """The bars of test_gpu_evidence.py (1e-8 of max |ref| against the closed forms of _evidence_reference.py on the device's Gram
    matrix, the quadratic form at `_quad_slack`, log det at 1e-9) and of test_gpu_cv.py (`hold`: RATIO x the float64 yardstick
    from the long-double evaluation on the device's factor)."""
    import _cv_reference as cv
    import _evidence_reference as er
    import test_gpu_cv as CV
    import test_gpu_evidence as EV
    o, r, y = res.out, res.ref.r, res.ref.y
    n0, n = res.ref.blocks[0], sum(res.ref.blocks)
    G = gram(ctx, res.ref.X, res.ref.noise, res.ref.blocks)
    check_factor(G, o["L"], name)
    Ginv = np.linalg.inv(G)
    w = Ginv @ r
    EV._close(np.tril(o["inverse"]), np.tril(Ginv), f"{name} inverse")
    EV._close(o["inverse_diag"], er.inverse_diag(G), f"{name} inverse_diag")
    quad, logdet, _ = er.evidence(G, r)
    slack, _ = EV._quad_slack(G, r, w)
    assert abs(o["evidence"][0] - quad) <= slack and abs(o["evidence"][1] - logdet) <= 1e-9 * abs(logdet), (name, o["evidence"], quad, logdet)
    mean, var, logp = er.loo(G, r, y)
    EV._close(o["loo.mean"], mean, f"{name} loo mean")
    EV._close(o["loo.var"], var, f"{name} loo var")
    EV._close(o["loo.logp"], logp, f"{name} loo logp")
    EV._close(o["loo.total"], np.array([np.sum(logp)]), f"{name} loo total")
    dG = np.tril(o["dG"]) + np.tril(o["dG"], -1).T
    EV._close(o["grad"], np.array([w @ dG @ w, np.sum(Ginv * dG)]), f"{name} evidence_grad")
    d = np.zeros(n)
    d[n0:] = res.ref.v + res.ref.scalar
    EV._close(o["grad_diag"], np.array([w @ (d * w), np.sum(np.diag(Ginv) * d)]), f"{name} evidence_grad_diag")
    fold_of, nfolds = S.f_folds(n)
    folds = [np.flatnonzero(fold_of == f) for f in range(nfolds)]
    ref, lap = cv.evaluate(o["L"], r, y, folds), cv.evaluate_float64(o["L"], r, y, folds)
    for key, got, a, b in (("mean", o["cv.mean"], lap.mean, ref.mean), ("var", o["cv.var"], lap.var, ref.var), ("logp", o["cv.logp"], lap.logp, ref.logp),
                           ("total", o["cv.total"], [lap.total], [ref.total])):
        CV.hold(f"{name} cv {key}", got, a, b)
    for f in range(nfolds):
        CV.hold(f"{name} cv cov {f}", o[f"cv.cov{f}"], lap.cov[f], ref.cov[f])


def reference_h(ctx, name, res):
    """The posterior criterion of conftest.py against the oracle, as test_gpu_fused.py holds the Kronecker path."""
    from conftest import assert_posterior_close
    from oracle import covfuncs as ocf
    from oracle import gp as ogp
    post = ogp.condition([S.H_KERNEL], [ogp.ObsBlock(res.ref.X, ocf.identity(2), res.ref.Y, 0.0, 1e-2)])
    assert_posterior_close(res.out["mean"], res.out["var"], post.mean(res.ref.Xt), post.var(res.ref.Xt))
    L = res.out["L"]
    np.testing.assert_allclose(L @ L.T, post.G, rtol=0, atol=1e-12 * np.max(np.abs(post.G)) * 4)


def reference_h_operator(ctx, name, res):
    """The assembled block entry by entry at the bound of test_gpu_varcoef.py / test_gpu_mixed.py against their dense references, the
    factor and the prediction at the bars of every other workload."""
    import test_gpu_mixed as MX
    import test_gpu_varcoef as VC
    G0, X1 = res.out["G0"], res.ref.X1
    if name == "h_weighted":
        ref, env, absw = VC.vr.block(VC._KERNEL2, VC._OP3, VC._OP3, X1, X1)
        ratio = np.abs(G0 - ref) / VC._entry_bound(env, absw, 9)
        assert ratio.max() <= 1.0, f"{name}: worst entry at {ratio.max():.3f} of its bound"
    else:
        MX._hold(name, G0, *MX.mr.block(MX._kernel(2), MX._lap(2), MX._lap(2), X1, X1, res.ref.A1, res.ref.A1), 9, 9)
    assert np.array_equal(G0, G0.T)
    check_factor(res.out["G"], res.out["L"], name)
    # V at the LAPACK-relative bar of test_gpu_predict_backward.check_V.  Its second bar, CEIL n eps, is 1.3 eps at these 130 rows:
    # below LAPACK's own componentwise backward error on this L and K0 (measured 1.6 - 1.7 eps; the device's is 0.78 of it), so it
    # says nothing here and is not applied.  The read-outs at the bar of the two files this workload is taken from: the posterior
    # criterion of conftest.py against a LAPACK solve on the device's own G and K0.
    import test_gpu_predict_backward as PB
    from conftest import assert_posterior_close
    c = res.ref.case
    cols = PB.columns(c.m)
    be = float(np.max(PB.cw_error(c.L, c.K0[:, cols], c.V[:, cols])))
    be_ref = float(np.max(PB.cw_error(c.L, c.K0[:, cols], scipy.linalg.solve_triangular(c.L, c.K0[:, cols], lower=True))))
    print(f"[V {name}] backward error {be:.3e} (LAPACK {be_ref:.3e}): ratio {be / max(be_ref, EPS):.2f}")
    assert be <= PB.RATIO * max(be_ref, EPS), f"{name}: V backward error {be:.3e}, LAPACK's {be_ref:.3e}"
    PB.check_var(c, name)
    G = np.tril(res.out["G"]) + np.tril(res.out["G"], -1).T
    cho = scipy.linalg.cho_factor(G, lower=True)
    mean_ref = c.K0.T @ scipy.linalg.cho_solve(cho, c.r)
    var_ref = c.kxx - np.sum(c.K0 * scipy.linalg.cho_solve(cho, c.K0), axis=0)
    assert_posterior_close(c.mean, c.var, mean_ref, var_ref)


def reference_i(ctx, name, res):
    """matvec: the device path equals the host-vector path bit for bit, and that path the long-double product at the bound of
    test_matvec_on_resident_blocks_equals_the_host_vector_path; pivchol: held inside the walk; PCG: every step within the running
    bounds of _pcg_reference.py from the device's own state, as test_each_step_against_the_reference_from_the_device_state."""
    import _pcg_reference as ref
    import test_gpu_pcg_kernels as PK
    if name == "i_pivchol":
        fig = res.ref.fig
        assert max(fig["L"], fig["d"], fig["delta"], fig["S"]) <= 1.0, fig
        return
    if name == "i_matvec":
        K = res.out["K"]
        tiles_r, tiles_c = -(-PK.MV_N0 // 64), -(-PK.MV_N1 // 64)
        splits = max(1, min(-(-4 * ctx.device_info()["cus"] // tiles_r), tiles_c))
        depth = tiles_c * 16 + splits + 4
        for m in (1, 9):
            Vh, old = res.ref.V[m], res.ref.old[m]
            for v_off, y_off in PK.MV_OFFSETS:
                want = res.out[f"host.m{m}.v{v_off}"]
                Vs = Vh[v_off:v_off + PK.MV_N1]
                err = np.abs(want.astype(LD) - K.astype(LD) @ Vs.astype(LD)).astype(np.float64)
                assert np.all(err <= 2 * depth * EPS / 2 * (np.abs(K) @ np.abs(Vs))), (name, m, v_off)
                rows = slice(y_off, y_off + PK.MV_N0)
                keep = np.ones(PK.MV_N, dtype=bool)
                keep[rows] = False
                for acc in (0, 1):
                    got = res.out[f"dev.m{m}.v{v_off}.y{y_off}.acc{acc}"]
                    assert PK.same_bits(got[rows], old[rows] + want if acc else want) and PK.same_bits(got[keep], old[keep]), (name, m, v_off, y_off, acc)
        return
    n, m, rank = res.ref.shape
    pb = ref.problem(n, m, rank)
    pre, bn = pb.preconditioner(), ref.bnorm(pb.B)
    for k in range(ref.STEPS):
        Xh, Rh, Zh, Ph = res.ref.before[k]
        st = ref.state(pre, Xh, Rh, Zh, Ph, bn, PK.RTOL)
        new, bd = ref.step(pre, st, res.ref.Q[k], PK.RTOL)
        cond = max(*(float(np.max(v)) for v in st.cond.values()), *(float(np.max(v)) for v in new.cond.values()))
        assert cond <= ref.COND_MAX, cond
        for key in ("X", "R", "Z", "P", "rel"):
            ratio = ref.worst_ratio(res.out[f"step{k}.{key}"], getattr(new, key), bd[key])
            assert ratio <= 1.0, f"{name} step {k} {key}: {ratio:.3f} of its bound"


def reference(ctx, name, res):
    for prefix, fn in (("h_weighted", reference_h_operator), ("h_mixed", reference_h_operator), ("i_", reference_i), ("a_", reference_a), ("b_", reference_b), ("c_", reference_c), ("d_chain_", reference_d_chain), ("d_", reference_d),
                       ("e_", reference_e), ("f_", reference_f), ("g_", reference_g), ("h_", reference_h)):
        if name.startswith(prefix):
            return fn(ctx, name, res)
    raise KeyError(name)


# ---- the assertions every run is held to ---------------------------------------------------------------------------------
def check_run(name, fill, res):
    tag = f"{name} fill 0x{fill:02X}"
    kinds = set()
    assert res.log, f"{tag}: the workload recorded no proof of reuse"
    for kind, need, count, nbytes in res.log:
        least = len(kind.split("+"))             # (a proof around a whole workload: at least one buffer per object it stands for)
        assert count >= least and nbytes >= need, f"{tag}: {kind}: {count} buffers, {nbytes} bytes filled, {need} expected: the workload got round the pool"
        kinds |= set(kind.split("+"))
    if not name.startswith("i_"):                # (the matrix-free paths hold no matrix)
        assert "matrix" in kinds and (kinds & {"rhs", "buffers"}), f"{tag}: no filled matrix and right-hand side on record ({kinds})"
    for key, arr in res.out.items():
        assert np.all(np.isfinite(arr)), f"{tag}: {key} is not finite ({int(np.sum(~np.isfinite(arr)))} entries)"
    for key, (raw, blocks, factored) in res.raws.items():
        bad = S.contract_violations(raw, blocks, factored)
        assert not bad, f"{tag}: raw storage {key}: {len(bad)} violations of the padding contract, the first: {bad[:3]}"


def compare(name, fill, res, base):
    tag = f"{name} fill 0x{fill:02X}"
    assert res.out.keys() == base.out.keys() and res.raws.keys() == base.raws.keys(), tag
    for key in res.out:
        a, b = np.asarray(res.out[key]), np.asarray(base.out[key])
        if not S.same_bits(a, b):
            where = ""
            if a.shape == b.shape:
                diff = (a != b) & ~(np.isnan(a) & np.isnan(b))
                where = f": {int(np.sum(diff))} entries, the first at {tuple(int(i) for i in np.argwhere(diff)[0])}" if diff.any() else ": NaN payloads or signs of zero"
            raise AssertionError(f"{tag}: {key} differs from the 0x00 run{where}")
    for key in res.raws:
        (a, blocks, factored), (b, _, _) = res.raws[key], base.raws[key]
        mask = S.defined_mask(a.shape[0], factored)
        am, bm = np.where(mask, a, 0.0), np.where(mask, b, 0.0)
        if not S.same_bits(am, bm):
            diff = (am != bm) | (np.isnan(am) != np.isnan(bm))
            raise AssertionError(f"{tag}: raw storage {key} differs from the 0x00 run where the contract defines it: {int(np.sum(diff))} entries, "
                                 f"the first at {tuple(int(i) for i in np.argwhere(diff)[0]) if diff.any() else 'payload only'}")


@pytest.mark.parametrize("fill", S.FILLS, ids=[f"0x{f:02X}" for f in S.FILLS])
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_workload(ctx, name, fill):
    try:
        if name not in _base:
            _base[name] = run(ctx, name, S.FILLS[0])
        base = _base[name]
        if fill == S.FILLS[0]:
            check_run(name, fill, base)
            reference(ctx, name, base)
        else:
            res = run(ctx, name, fill)
            check_run(name, fill, res)
            compare(name, fill, res, base)
    finally:
        if fill == S.FILLS[-1]:
            _base.pop(name, None)


def test_the_mode_is_off_by_default_and_off_fills_nothing(ctx):
    """Without the hook no buffer is filled: a conditioning and a prediction leave `filled` at (0, 0)."""
    assert _hooks.set_pool_fill(ctx, -1) == (0, 0)
    X, noise = S.observation_points(130)
    ap = Appender(ctx, X, noise)
    ap.add(130)
    assert ap.mat.potrf() == 0
    assert np.all(np.isfinite(ap.mat.solve_weights(np.ones(130))))
    assert _hooks.set_pool_fill(ctx, -1) == (0, 0)
    with _hooks.pool_fill(ctx, 0xFF) as take:
        take()
        ap2 = Appender(ctx, X, noise)
        count, nbytes = take()
        assert count >= 3 and nbytes >= 8 * 256 * 256           # a | linv | w
        del ap2
    assert _hooks.set_pool_fill(ctx, -1) == (0, 0)              # (switched off by the context manager, which took the rest)


def test_the_hook_refuses_a_context_of_a_multi_gpu_job(ctx):
    """A second context on the same device that has joined a job of one rank over the host-staged transport is distributed (as
    test_gpu_pivchol.py makes one): the hook refuses it, on and off, and leaves the first context's mode alone."""
    from linpde_gp_amd import _engine, _lib
    ctx2 = _engine.Context(ctx.device)
    try:
        exchange = _lib.HOST_EXCHANGE_FN(lambda user, op, buf, nbytes, root: 0)
        _lib.check(_lib.lib.lpgp_dist_init_host(ctx2._h, 0, 1, exchange, None), "lpgp_dist_init_host")
        for byte in (0, 0xFF, -1):
            with pytest.raises(_lib.LpgpError, match="single GPU only"):
                _hooks.set_pool_fill(ctx2, byte)
    finally:
        ctx2.close()
    assert _hooks.set_pool_fill(ctx, -1) == (0, 0)
