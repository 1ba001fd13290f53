"""The sharded Cholesky and its streamed solves (csrc/dist.hip: potrf_dist, panel_rows_solve, factor_diag_block, update_local,
trsm_lower_dist, trsm_lower_t_dist, factor_to_host_dist) held to the bars of the single-GPU suite test_gpu_potrf_backward.py
(`RATIO`, `CEIL`, `RATIO_SOLVE`, `check_factor`) on multi-rank jobs whose ranks share the one GPU.  No bar is set here and none is
raised: the sharded path runs the same tile kernels.

One job per row of `JOBS`, all cases inside it.  The parent writes the inputs (.npy, job.json) into a temporary directory, forms the
single-GPU references in its own context while no rank runs, starts the ranks (tests/_dist_backward_worker.py: fresh processes,
device work only, the environment of test_gpu_dist._run_ranks) and runs every check itself; rank 0 writes the result arrays, every rank
the SHA-256 of each result -- all ranks must hold the same bits.

  dense     kinds (a), (b), (c) of test_gpu_potrf_backward.matrix, entered by the Zero kernel and add_dense, factored twice (bit
            identity), collected factor finite with zeros above the diagonal, factor_diag() -- local, from the replicated diagonal
            blocks -- bitwise diag(L) on every rank, the bars of check_factor, and the row-scaled distance from the single-GPU
            factor of the same matrix at the same nb at most RATIO x LAPACK's distance from it (the bar of test_appends);
  solves    potrs with 1, 9 and 900 right-hand sides and solve_weights on dense (b): normwise backward error at most RATIO_SOLVE x
            cho_solve's on the same A, b.  900 columns pad to 1024 = 8 tile columns: mtl = 8, the look-ahead branch of
            trsm_lower_dist (`mtl >= 8`); run again with lookahead = 0, both held to the bar.  For 900 columns the long-double
            residual is formed on the columns `columns(900)` of test_gpu_predict_backward.py (one of every 16, the edges), and the
            residual of ALL 900 columns in float64 (see `test_solves`);
  pivots    kind (a) broken by `broken(A, L, k)` at k in {1, 129, nb + 1, 2 nb + 1, last ragged tile + 1, n}: every rank reports
            info == k -- the FIRST bad pivot, though the blocks behind it fail in their turn on other ranks --; after pop_block the
            corrected block factors in the same matrix and meets the bars.

No job here appends a block to a factored matrix or lets a sharded matrix grow (one block of n rows in a matrix created for n rows):
lpgp_mat_add_block growing a sharded matrix (mat_alloc, csrc/api.hip) has ended in a GPU memory fault on 3 x 1 and 2 x 2 grids and
the cause is not known.  So the old-panel phase of potrf_dist, the b0 > 0 path of factor_diag_block, trsm_lower() on an assembled
right-hand side and a pivot broken in an appended block are NOT covered by this file, on any grid.

Largest measured values (MI355X, all six jobs, in brackets): the sharded factor's backward error is [4.65] x LAPACK's, [0.001] n eps
and [1.15] x the single-GPU factor's on the same matrix; its row-scaled distance from the single-GPU factor is [0.23] x LAPACK's
distance from it.  The solves: [1.13] x cho_solve's normwise backward error in long double (look-ahead on and off: the same
figures), [1.03] x in float64 over all 900 columns.

A rank that ends by a signal, with status 134 / 139, or at the time limit: the other ranks are killed, the test fails with the tails
of the outputs, and the rest of this file skips instead of starting further GPU jobs."""
import concurrent.futures
import json
import os
import subprocess
import sys
import time
import types
from collections import namedtuple

import numpy as np
import pytest
import scipy.linalg

import test_gpu_potrf_backward as tb
import test_gpu_predict_backward as pb
from _backward import EPS, backward_error, restored, row_scaled_distance, solve_backward_error
from test_gpu_dist import _rccl_as_if_on_separate_hosts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_dist_backward_worker.py")

# seconds for one job.  Measured: the slowest job (2 x 1, nb 512, RCCL over loopback, n = 2125) takes 30 s from the first Popen to the
# last exit (the others 8 to 26 s: 2 x 2 over host 19 s, over the 1-MiB windows 26 s); five times that.
# (test_multi_rank_on_one_gpu_host_transport[(2, 2) ...] of the parent commit, one workload with five conditionings: under 5 s; a
# job here factors thirteen matrices of up to 2125 rows, collects seven factors and solves for 1811 right-hand sides.)
JOB_LIMIT_S = 150.0

Job = namedtuple("Job", "id grid nb transport n window_mb port")
JOBS = [
    Job("2x1-nb512-host", (2, 1), 512, "host", 2125, None, 30311),        # the default block width: split gather and look-ahead
    Job("1x2-nb256-host", (1, 2), 256, "host", 1333, None, 30321),        # n = 1333: 11 tiles, ragged last block, the layout wraps
    Job("3x1-nb128-host", (3, 1), 128, "host", 1333, None, 30331),
    Job("2x2-nb256-host", (2, 2), 256, "host", 1333, None, 30341),
    Job("2x2-nb256-ipc1", (2, 2), 256, "ipc", 1333, 1, 30351),            # 1-MiB windows: pieces travel in slices
    Job("2x1-nb512-rccl", (2, 1), 512, "rccl", 2125, None, 30361),        # RCCL over loopback sockets
]
NRHS = (1, 9, 900)           # 900 -> m_pad = 1024 = 8 * 128: mtl = 8, the smallest width that takes trsm_lower_dist's look-ahead

_cache = {}
_jobs = {}                  # job id -> Result, or the message of the failure that ended it
_trouble = []               # a rank faulted, aborted or hung: no further GPU job from this file


@pytest.fixture(scope="module")
def ctx():
    from linpde_gp_amd import _engine
    return _engine.default_context()


def single_factor(ctx, key, A, nb):
    """(factor, backward error) of A as ONE block on the single GPU at block width nb (the parent's context; no rank is running)."""
    k = ("single", key, A.shape[0], nb)
    if k not in _cache:
        with restored(ctx, ("nb",)) as apply:
            apply({"nb": nb})
            L = tb.factor(ctx, A).todense("factor")
        _cache[k] = (L, backward_error(A, L))
    return _cache[k]


def pivot_positions(n, nb):
    return sorted({1, 129, nb + 1, 2 * nb + 1, (n // 128) * 128 + 1, n})


class Result:
    def __init__(self, job, work, seconds, ranks):
        self.job, self.work, self.seconds, self.ranks = job, work, seconds, ranks

    def arr(self, name):
        return np.load(os.path.join(self.work, "out", name + ".npy"))

    def same_bits(self, name):
        """Every rank holds the same bits of result `name`; returns the array rank 0 wrote."""
        hashes = {r["sha:" + name] for r in self.ranks}
        assert len(hashes) == 1, f"{self.job.id}: the ranks hold different bits of {name}"
        return self.arr(name)

    def every(self, key):
        vals = [r[key] for r in self.ranks]
        assert all(v == vals[0] for v in vals), f"{self.job.id}: the ranks disagree on {key}: {vals}"
        return vals[0]


def write_inputs(ctx, job, work):
    """Inputs of the job as .npy and job.json; the single-GPU references are formed here (no rank runs yet)."""
    n, nb = job.n, job.nb
    os.makedirs(os.path.join(work, "out"))
    save = lambda name, a: np.save(os.path.join(work, name + ".npy"), a)
    cases = []
    for kind in "abc":
        save("A_" + kind, tb.matrix(kind, n))
        cases.append({"case": "dense", "tag": "dense_" + kind, "matrix": "A_" + kind, "solves": kind == "b"})
    rng = np.random.default_rng(n + 17)
    for nrhs in NRHS:
        save(f"rhs_{nrhs}", rng.standard_normal((n, nrhs)))
    save("r", np.random.default_rng(n + 1).standard_normal(n))
    A = tb.matrix("a", n)
    L = tb.lapack(A)[0]
    cases.append({"case": "pivot_dense", "tag": "pivot_a", "matrix": "A_a",
                  "breaks": [[k, float(tb.broken(A, L, k)[k - 1, k - 1])] for k in pivot_positions(n, nb)]})
    with open(os.path.join(work, "job.json"), "w") as f:
        json.dump({"grid": list(job.grid), "nb": nb, "transport": job.transport, "n": n, "nrhs": list(NRHS), "cases": cases}, f)
    # the single-GPU factors the sharded ones are compared with
    for kind in "abc":
        single_factor(ctx, kind, tb.matrix(kind, n), nb)


def run_ranks(job, work):
    """Starts the ranks and waits for them, at most JOB_LIMIT_S; the first rank that ends badly ends the job.  Returns seconds."""
    world = job.grid[0] * job.grid[1]
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(job.port), LPGP_DEVICE="0")
    env.pop("LOCAL_RANK", None)
    env.update(OPENBLAS_NUM_THREADS="4", OMP_NUM_THREADS="4", MKL_NUM_THREADS="4")
    if job.window_mb is not None:
        env["LPGP_IPC_WINDOW_MB"] = str(job.window_mb)
    rank_env = _rccl_as_if_on_separate_hosts if job.transport == "rccl" else (lambda r: {})
    files = [(open(os.path.join(work, f"rank{r}.out"), "w+"), open(os.path.join(work, f"rank{r}.err"), "w+")) for r in range(world)]
    t0 = time.monotonic()
    procs = [subprocess.Popen([sys.executable, WORKER, work], env=dict(env, RANK=str(r), **rank_env(r)), stdout=files[r][0], stderr=files[r][1],
                              text=True) for r in range(world)]
    timed_out, trigger = False, 0          # trigger: the first status that was not 0
    pool = concurrent.futures.ThreadPoolExecutor(world)
    try:
        pending = {pool.submit(p.wait) for p in procs}
        while pending and not timed_out and trigger == 0:
            done, pending = concurrent.futures.wait(pending, timeout=max(0.0, t0 + JOB_LIMIT_S - time.monotonic()),
                                                    return_when=concurrent.futures.FIRST_COMPLETED)
            timed_out = not done
            trigger = next((f.result() for f in done if f.result() != 0), 0)
    finally:
        for p in procs:                                # the job is over: a peer of a dead rank would wait for its pieces
            if p.poll() is None:
                p.kill()
            p.wait()
        pool.shutdown()
    seconds = time.monotonic() - t0
    tails = []
    for r, (fo, fe) in enumerate(files):
        fo.seek(0)
        fe.seek(0)
        tails.append((fo.read(), fe.read()))
        fo.close()
        fe.close()
    codes = [p.returncode for p in procs]
    report = "".join(f"\n--- rank {r} (status {codes[r]}) ---\n{so[-1500:]}\n{se[-3000:]}" for r, (so, se) in enumerate(tails))
    if job.transport == "rccl" and any("lpgp_dist_init failed" in so + se or "lpgp_dist_unique_id failed" in so + se for so, se in tails):
        return None, "RCCL could not be brought up over loopback sockets here: " + (tails[0][0] + tails[0][1])[-300:]
    faulted = any("illegal memory access" in so + se or "Memory access fault" in so + se for so, se in tails)
    if timed_out or faulted or trigger in (134, 139) or trigger < 0:      # a limit, a GPU fault, an abort, a segmentation fault, a signal
        _trouble.append(f"job {job.id}: " + ("time limit" if timed_out else f"statuses {codes}"))
    if timed_out:
        raise AssertionError(f"job {job.id}: not finished after {JOB_LIMIT_S:.0f} s, ranks killed" + report)
    assert all(c == 0 for c in codes), f"job {job.id}: statuses {codes}" + report
    for r, (so, _) in enumerate(tails):
        assert f"RANK {r} of {world} DONE" in so, report
    return seconds, None


def result_of(ctx, job, tmp_path_factory):
    if job.id in _jobs:
        got = _jobs[job.id]
        if isinstance(got, Result):
            return got
        if got.startswith("skip:"):
            pytest.skip(got[5:])
        pytest.fail("the job of this case failed: " + got[:600])
    if _trouble:
        pytest.skip("a rank of an earlier job of this file faulted, aborted or hung -- no further GPU jobs: " + _trouble[0])
    work = str(tmp_path_factory.mktemp("dist-" + job.id))
    write_inputs(ctx, job, work)
    try:
        seconds, skip = run_ranks(job, work)
    except AssertionError as exc:
        _jobs[job.id] = str(exc)
        raise
    if skip:
        _jobs[job.id] = "skip:" + skip
        pytest.skip(skip)
    world = job.grid[0] * job.grid[1]
    ranks = []
    for r in range(world):
        with open(os.path.join(work, "out", f"rank{r}.json")) as f:
            ranks.append(json.load(f))
    print(f"\n[dist {job.id}] job of {world} ranks took {seconds:.1f} s")
    _jobs[job.id] = Result(job, work, seconds, ranks)
    return _jobs[job.id]


@pytest.fixture(params=JOBS, ids=[j.id for j in JOBS])
def res(request, ctx, tmp_path_factory):
    return result_of(ctx, request.param, tmp_path_factory)


# ---- checks ------------------------------------------------------------------------------------------------------------------
def factor_checks(ctx, res, tag, A, single_key):
    """The collected factor `L_<tag>`: bits, the bars of check_factor, the distance from the single-GPU factor."""
    job = res.job
    assert res.every("info:" + tag) == 0 and res.every("info2:" + tag) == 0
    L = res.same_bits("L_" + tag)
    for r in res.ranks:
        assert r["sha:L2_" + tag] == r["sha:L_" + tag], f"{job.id} {tag}: two factorisations of the same matrix differ"
        assert r["diag:L_" + tag], f"{job.id} {tag}: factor_diag() is not the diagonal of the collected factor"
    shim = types.SimpleNamespace(todense=lambda what: L, factor_diag=lambda: np.diag(L))
    be, ratio, _ = tb.check_factor(shim, A, f"{job.id} {tag}")
    L1, be1 = single_factor(ctx, single_key, A, job.nb)
    d_dev, d_lap = row_scaled_distance(A, L, L1), row_scaled_distance(A, tb.lapack(A)[0], L1)
    print(f"[dist {job.id} {tag}] backward error {be:.3e} = {be / max(be1, 1e-3 * EPS):.2f} x single-GPU's {be1:.3e} ({ratio:.2f} x LAPACK's); "
          f"|L_sharded - L_single| = {d_dev:.3e}, |L_lapack - L_single| = {d_lap:.3e} (row-scaled): {d_dev / max(d_lap, EPS):.2f}")
    assert d_dev <= tb.RATIO * max(d_lap, EPS), f"{job.id} {tag}: sharded and single-GPU factor differ by {d_dev:.3e} (LAPACK: {d_lap:.3e})"


def test_dense_factors(ctx, res):
    for kind in "abc":
        factor_checks(ctx, res, "dense_" + kind, tb.matrix(kind, res.job.n), kind)


def cho_solution(A, key, b):
    """cho_solve's solution of A x = b (cached: two jobs share a size)."""
    k = ("cho", id(A), key)
    if k not in _cache:
        _cache[k] = scipy.linalg.cho_solve((tb.lapack(A)[0], True), b)
    return _cache[k]


def error_f64(A, x, b):
    """The quantity of `solve_backward_error` with the residual in float64 (BLAS): cheap enough for every column."""
    nA = float(np.max(np.sum(np.abs(A), axis=1)))
    return float(np.max(np.abs(A @ x - b))) / (nA * float(np.max(np.abs(x))) + float(np.max(np.abs(b))))


def test_solves(res):
    """The bar is held in long double; for 900 columns that residual is formed on the sampled columns only (a long-double product of
    all of them takes tens of seconds).  Every tile column is sampled, but an error local to one unsampled column would pass, so the
    residual of ALL columns is formed in float64 as well and held to the same ratio against cho_solve's, formed the same way: there
    the evaluation's own rounding, the same for both, hides a lost digit, but not a wrong column."""
    job, n = res.job, res.job.n
    rng = np.random.default_rng(n + 17)
    rhs = {nrhs: rng.standard_normal((n, nrhs)) for nrhs in NRHS}          # (as write_inputs drew them)
    r = np.random.default_rng(n + 1).standard_normal((n, 1))
    wide = max(NRHS)
    cols = pb.columns(wide)
    tag, A = "dense_b", tb.matrix("b", n)
    # (result, what, right-hand side, key of the reference)
    runs = [(f"x_{tag}_{nrhs}", f"nrhs={nrhs}", rhs[nrhs], nrhs) for nrhs in NRHS]
    runs.append((f"x_{tag}_{wide}_la0", f"nrhs={wide} lookahead=0", rhs[wide], wide))
    runs.append((f"w_{tag}", "solve_weights", r, "r"))
    for name, what, b, key in runs:
        x = res.same_bits(name).reshape(b.shape)
        xref = cho_solution(A, key, b)
        assert np.all(np.isfinite(x)), f"{job.id} {tag} {what}"
        if key == wide:
            e64, ref64 = error_f64(A, x, b), error_f64(A, xref, b)
            print(f"[dist {job.id} {tag}] {what}: all columns in float64: {e64:.3e} (cho_solve {ref64:.3e}): ratio {e64 / ref64:.2f}")
            assert e64 <= tb.RATIO_SOLVE * ref64, f"{job.id} {tag} {what}: all columns, float64: {e64:.3e} vs cho_solve {ref64:.3e}"
            x, xref, b = x[:, cols], xref[:, cols], b[:, cols]
        err, ref = solve_backward_error(A, x, b), solve_backward_error(A, xref, b)
        print(f"[dist {job.id} {tag}] {what}: backward error {err:.3e} (cho_solve {ref:.3e}): ratio {err / ref:.2f}")
        assert err <= tb.RATIO_SOLVE * ref, f"{job.id} {tag} {what}: {err:.3e} vs cho_solve {ref:.3e}"


def test_first_bad_pivot(ctx, res):
    """A bad pivot is seen by the owner of its diagonal block; the blocks behind it fail in their turn on their owners.  The job's
    status is the first of them on every rank (potrf_dist: the smallest positive status)."""
    job, n = res.job, res.job.n
    ks = pivot_positions(n, job.nb)
    assert res.every("info:pivot_a") == ks, f"{job.id}: first bad pivots {res.every('info:pivot_a')}, broken at {ks}"
    assert res.every("info_after:pivot_a") == 0
    A = tb.matrix("a", n)
    L = res.same_bits("L_pivot_a")
    assert all(r["diag:L_pivot_a"] for r in res.ranks)
    tb.check_factor(types.SimpleNamespace(todense=lambda what: L, factor_diag=lambda: np.diag(L)), A, f"{job.id} after failure a")
