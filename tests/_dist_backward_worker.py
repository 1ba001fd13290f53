"""One rank of a job of tests/test_gpu_dist_backward.py: a plain script, started once per rank by the test (RANK / WORLD_SIZE /
MASTER_* in the environment, the job's directory as its argument).  Device work only -- no LAPACK, no long double: the inputs come
as .npy files from the parent (job.json lists the cases), rank 0 writes every result array into <dir>/out, and EVERY rank writes the
SHA-256 of every result (and the statuses it saw) into <dir>/out/rank<r>.json.  The parent runs all the checks."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "linpde-gp_amd"))

import numpy as np  # noqa: E402

from linpde_gp_amd import _dist, _engine  # noqa: E402
from linpde_gp_amd.randprocs import covfuncs  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    work = sys.argv[1]
    with open(os.path.join(work, "job.json")) as f:
        job = json.load(f)
    comm = _dist.Comm.from_env()
    ctx = _engine.default_context()            # LPGP_DEVICE=0 on every rank: the ranks share the GPU
    ctx.set_option("nb", job["nb"])
    ctx.dist_init(comm, transport=job["transport"], grid=tuple(job["grid"]))
    assert ctx.world == comm.world and ctx.grid == tuple(job["grid"])
    out = os.path.join(work, "out")
    res = {}

    def load(name):
        return np.load(os.path.join(work, name + ".npy"))

    def keep(name, arr):
        res["sha:" + name] = sha(arr)
        if comm.rank == 0:
            np.save(os.path.join(out, name + ".npy"), arr)

    def new_matrix(A):
        """One block, cleared by the Zero kernel, then A added (test_gpu_potrf_backward.new_matrix)."""
        n = A.shape[0]
        mat = _engine.GramMatrix(ctx, n)
        fill(mat, A)
        return mat

    def fill(mat, A):
        n = A.shape[0]
        bi = mat.add_block(n)
        mat.assemble(covfuncs.Zero(()).lower(), _engine.Points(ctx, np.zeros((n, 1))), None, bi, bi)
        mat.add_dense(bi, A)

    def collected(mat, name):
        """The factor collected on every rank (kept under `name`) and whether the local diagonal -- from the replicated diagonal
        blocks -- is the collected one bit for bit."""
        L = mat.todense("factor")
        res["diag:" + name] = bool(np.array_equal(mat.factor_diag(), np.diag(L)))
        keep(name, L)
        return L

    def solves(mat, tag):
        for nrhs in job["nrhs"]:
            B = load(f"rhs_{nrhs}")
            keep(f"x_{tag}_{nrhs}", mat.potrs(B[:, 0] if nrhs == 1 else B).reshape(B.shape))
        wide = max(job["nrhs"])
        lookahead = ctx.get_option("lookahead")
        ctx.set_option("lookahead", 0)
        try:
            keep(f"x_{tag}_{wide}_la0", mat.potrs(load(f"rhs_{wide}")))
        finally:
            ctx.set_option("lookahead", lookahead)
        keep(f"w_{tag}", mat.solve_weights(load("r")))

    for case in job["cases"]:
        what, tag = case["case"], case["tag"]
        if what == "dense":
            A = load(case["matrix"])
            mat = new_matrix(A)
            res["info:" + tag] = mat.potrf()
            collected(mat, "L_" + tag)
            mat2 = new_matrix(A)
            res["info2:" + tag] = mat2.potrf()
            res["sha:L2_" + tag] = sha(mat2.todense("factor"))
            del mat2
            if case.get("solves"):
                solves(mat, tag)
            del mat
        elif what == "pivot_dense":
            A = load(case["matrix"])
            infos = []
            for k, value in case["breaks"]:
                B = A.copy()
                B[k - 1, k - 1] = value                      # (test_gpu_potrf_backward.broken: formed by the parent)
                mat = new_matrix(B)
                infos.append(mat.potrf())
                mat.pop_block()
            res["info:" + tag] = infos
            fill(mat, A)                                     # a corrected block then factors in the matrix that failed
            res["info_after:" + tag] = mat.potrf()
            collected(mat, "L_" + tag)
            del mat
        else:
            raise SystemExit(f"unknown case {what}")
    with open(os.path.join(out, f"rank{comm.rank}.json"), "w") as f:
        json.dump(res, f)
    comm.barrier()
    comm.close()
    print("RANK", comm.rank, "of", comm.world, "DONE", flush=True)


if __name__ == "__main__":
    main()
