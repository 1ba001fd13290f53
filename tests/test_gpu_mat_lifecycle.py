"""The life cycle of a matrix handle through the C ABI: the host bookkeeping of `lpgp_mat` (csrc/mat_state.h: block table and
factor state) seen from outside.  One walk -- lazy conditioning, a failed status, `check`, `truncate`, re-conditioning, `predict`, a
view round trip, a clone of a prefix extended by a block -- whose every prediction must equal, bit for bit, the same prediction
of a matrix that went through the same calls and never failed.  tests/test_mat_state_host.py walks the same transitions on the
host alone; the negative status (a timed-out hand-over) is held by tests/test_gpu_chain.py.

Blocks of 1, 128 and 129 rows (padded offsets 0, 128, 256; 512 padded rows): pivot 130 is row 129 of the padded order, the
second row of block 1."""
import numpy as np
import pytest

import _hooks
from _backward import Appender, gram_points

pytestmark = pytest.mark.gpu

BLOCKS = [1, 128, 129]
N = sum(BLOCKS)
M = 3                       # test points


def _predict(ctx, ap, Xt, kxx, r):
    """Mean and variance at `Xt` from the blocks in view through `lpgp_potrf_predict`: what is not factored yet is factored on the way."""
    from linpde_gp_amd import _engine
    K = _engine.Rhs(ctx, ap.mat, M)
    for bi in range(ap.mat.num_blocks):
        K.cross_assemble(ap.kd, ap.pts[bi], Xt, bi)
    ap.mat.set_residual(r[:ap.mat.n])
    return K.potrf_predict(None, kxx)


def _walk(ctx, X, noise, Xt, kxx, r, fail):
    """The predictions of the walk, in order: after the (re-)conditioning, after the view round trip, from the extended clone."""
    ap = Appender(ctx, X, noise)
    mat = ap.mat
    ap.add(BLOCKS[0])
    mat.potrf_enqueue()
    if fail:
        for nb in BLOCKS[1:]:                          # lazily: enqueued, the status not read
            ap.add(nb)
            mat.potrf_enqueue()
        _hooks.force_status(ctx, mat, 130)
        assert mat.check() == (130, 1)
        assert mat.check() == (0, -1)                  # reported once: a positive status is a rollback, not a dead matrix
        assert (mat.n, mat.padded_n, mat.num_blocks) == (N, 512, 3)
        ap.drop(1, truncate=True)
        assert (mat.n, mat.padded_n, mat.num_blocks) == (1, 128, 1)
        assert mat.check() == (0, -1)
    for nb in BLOCKS[1:]:
        ap.add(nb)                                     # assembled only: the prediction factors them
    out = [_predict(ctx, ap, Xt, kxx, r)]
    assert mat.check() == (0, -1)                      # the status read back with the results
    assert (mat.n, mat.padded_n, mat.num_blocks, mat.num_blocks_total) == (N, 512, 3, 3)
    mat.set_view(1)
    assert (mat.n, mat.padded_n, mat.num_blocks, mat.num_blocks_total) == (1, 128, 1, 3)
    mat.set_view(-1)
    assert (mat.n, mat.padded_n, mat.num_blocks, mat.num_blocks_total) == (N, 512, 3, 3)
    out.append(_predict(ctx, ap, Xt, kxx, r))
    ap2 = Appender(ctx, X, noise)
    ap2.mat = mat.clone(2)
    ap2.pts = list(ap.pts[:2])
    assert (ap2.mat.n, ap2.mat.padded_n, ap2.mat.num_blocks) == (BLOCKS[0] + BLOCKS[1], 256, 2)
    ap2.add(BLOCKS[2])
    out.append(_predict(ctx, ap2, Xt, kxx, r))
    assert ap2.mat.check() == (0, -1)
    assert (mat.n, mat.padded_n, mat.num_blocks) == (N, 512, 3)        # the source of the clone is as it was
    return out


def test_a_failed_block_rolled_back_leaves_the_matrix_as_if_it_never_failed():
    from linpde_gp_amd import _engine
    ctx = _engine.default_context()
    X, noise = gram_points("m", N)                     # unit noise: condition number at most 1 + N
    rng = np.random.default_rng(11)
    r = rng.standard_normal(N)
    xt = rng.uniform(0, 1, (M, 2))
    Xt = _engine.Points(ctx, xt)
    ap0 = Appender(ctx, X, noise)
    kxx = np.full(M, _engine.kernel_diag(ctx, ap0.kd))
    failed = _walk(ctx, X, noise, Xt, kxx, r, True)
    clean = _walk(ctx, X, noise, Xt, kxx, r, False)
    for step, ((m1, v1), (m0, v0)) in enumerate(zip(failed, clean)):
        assert np.array_equal(m1, m0) and np.array_equal(v1, v0), f"prediction {step}: {m1 - m0}, {v1 - v0}"
    # ... and the predictions are the posterior's: the device's own kernel matrices through a host solve.  With unit noise the
    # condition number is at most 1 + N = 259, the forward error of a backward-stable solve a few N eps cond ~ 1e-11 relative.
    P = _engine.Points(ctx, X)
    G = _engine.kernel_matrix(ctx, ap0.kd, P, P) + np.diag(noise)
    Kx = _engine.kernel_matrix(ctx, ap0.kd, P, Xt)
    mean = Kx.T @ np.linalg.solve(G, r)
    var = kxx - np.sum(Kx * np.linalg.solve(G, Kx), axis=0)
    for m1, v1 in failed:
        assert np.max(np.abs(m1 - mean)) <= 1e-9 * np.max(np.abs(mean))
        assert np.max(np.abs(v1 - var)) <= 1e-9 * kxx[0]
