"""Test hooks (include/lpgp_test.h, liblpgp_testhooks.so): raw kernels on host buffers, peak probes, the host replay of the
distributed tile enumeration.  TEST INFRASTRUCTURE -- the product package never loads this library
(`nm -D liblpgp.so | grep lpgp_test` is empty).  Used by tests/ and scratch/."""

from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np
import scipy.linalg

from linpde_gp_amd import _lib
from linpde_gp_amd._engine import Context
from linpde_gp_amd._lib import check

HOOKS_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "liblpgp_testhooks.so")

EXPORTED = ["lpgp_test_stair_enumerate", "lpgp_test_gemm", "lpgp_test_gemm_cyc", "lpgp_test_potrf_tile", "lpgp_test_tile_step", "lpgp_test_panel_solve",
            "lpgp_debug_tile_xcc", "lpgp_probe_mfma_f64", "lpgp_probe_hbm_write", "lpgp_test_force_status", "lpgp_test_solve_vec_fwd", "lpgp_test_solve_vec_bwd",
            "lpgp_test_trsm_lower_t", "lpgp_test_mat_raw", "lpgp_test_factor_matmul", "lpgp_test_evidence", "lpgp_test_loo", "lpgp_test_evidence_grad",
            "lpgp_test_evidence_grad_diag", "lpgp_test_pool_fill"]


def _load() -> C.CDLL:
    if not os.path.exists(HOOKS_PATH):
        raise ImportError(f"{HOOKS_PATH} not found (linpde-gp_amd/csrc/build.sh builds it next to liblpgp.so)")
    lib = C.CDLL(HOOKS_PATH)          # resolves its liblpgp.so through $ORIGIN: the library the package has already loaded
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    pd = C.POINTER(C.c_double)

    def sig(name, res, *args):
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = list(args)

    sig("lpgp_test_stair_enumerate", C.c_int, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32), i64)
    sig("lpgp_test_gemm", C.c_int, vp, i32, i32, i32, i64, i64, i64, dbl, pd, i64, pd, i64, dbl, pd, i64, i32, pd)
    sig("lpgp_test_gemm_cyc", C.c_int, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, dbl, dbl, pd, i64, pd, i64)
    sig("lpgp_test_potrf_tile", C.c_int, vp, pd, pd, C.POINTER(i32))
    sig("lpgp_debug_tile_xcc", C.c_int, vp, C.POINTER(i32), i32)
    sig("lpgp_test_tile_step", C.c_int, vp, i32, pd, i64, pd, pd, pd)
    sig("lpgp_test_panel_solve", C.c_int, vp, i32, pd, i32, i64, pd, pd, pd)
    sig("lpgp_probe_mfma_f64", C.c_int, vp, pd)
    sig("lpgp_probe_hbm_write", C.c_int, vp, i64, pd)
    sig("lpgp_test_force_status", C.c_int, vp, vp, i32)
    sig("lpgp_test_solve_vec_fwd", C.c_int, vp, vp, pd, pd)
    sig("lpgp_test_solve_vec_bwd", C.c_int, vp, vp, pd, pd)
    sig("lpgp_test_trsm_lower_t", C.c_int, vp, vp, pd, i64)
    sig("lpgp_test_mat_raw", C.c_int, vp, vp, i32, pd)
    sig("lpgp_test_factor_matmul", C.c_int, vp, vp, pd, i64, pd, pd, i32)
    sig("lpgp_test_evidence", C.c_int, vp, vp, pd, i32, pd)
    sig("lpgp_test_loo", C.c_int, vp, vp, pd, pd, i32, pd, pd, pd)
    sig("lpgp_test_evidence_grad", C.c_int, vp, vp, vp, vp, pd, i32, pd)
    sig("lpgp_test_evidence_grad_diag", C.c_int, vp, vp, vp, i32, pd, dbl, pd, i32, pd)
    sig("lpgp_test_pool_fill", C.c_int, vp, i32, C.POINTER(i64))
    return lib


lib = _load()


def probe_mfma_f64(ctx: Context) -> float:
    v = C.c_double()
    check(lib.lpgp_probe_mfma_f64(ctx._h, C.byref(v)), "lpgp_probe_mfma_f64")
    return v.value


def probe_hbm_write(ctx: Context, nbytes: int = 1 << 30) -> float:
    v = C.c_double()
    check(lib.lpgp_probe_hbm_write(ctx._h, int(nbytes), C.byref(v)), "lpgp_probe_hbm_write")
    return v.value


def test_gemm(ctx: Context, ta: int, tb: int, lower_only: int, alpha: float, A: np.ndarray, B: np.ndarray,
              beta: float, Cm: np.ndarray, k: int, reps: int = 0, m: int | None = None, n: int | None = None):
    """Raw GEMM on column-major (Fortran-ordered) arrays; returns (C, ms_per_rep).  The leading dimensions are the arrays' row
    counts; `m`, `n` (default: the shape of `Cm`) may be smaller than them, so a logical operand can sit inside a larger buffer."""
    A = np.asfortranarray(A, dtype=np.double)
    B = np.asfortranarray(B, dtype=np.double)
    Cm = np.asfortranarray(Cm, dtype=np.double).copy(order="F")
    m = Cm.shape[0] if m is None else int(m)
    n = Cm.shape[1] if n is None else int(n)
    # the hook uploads ld * (columns) elements of each buffer: they must exist
    a_cols, b_cols = (m if ta else k), (n if tb else k)
    if A.shape[1] < a_cols or B.shape[1] < b_cols or Cm.shape[1] < n or Cm.shape[0] < m:
        raise ValueError("test_gemm: a buffer is smaller than its logical operand")
    if A.shape[0] < (k if ta else m) or B.shape[0] < (k if tb else n):
        raise ValueError("test_gemm: a leading dimension is smaller than the logical rows")
    ms = C.c_double(0.0)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_gemm(ctx._h, ta, tb, lower_only, m, n, k, alpha,
                             A.ctypes.data_as(pd), A.shape[0], B.ctypes.data_as(pd), B.shape[0], beta,
                             Cm.ctypes.data_as(pd), Cm.shape[0], reps, C.byref(ms)), "lpgp_test_gemm")
    return Cm, ms.value


def test_gemm_cyc(ctx: Context, grid, rank, nbt: int, T: int, row_lo: int, col_lo: int, col_hi: int, g0: int, k: int, tri: int, occ3: int,
                  alpha: float, beta: float, panel: np.ndarray, Cm: np.ndarray) -> np.ndarray:
    """The trailing update of rank `rank` = (my_r, my_c) of the process grid `grid` = (pr, pc) as `potrf_dist` launches it
    (`lpgp_test_gemm_cyc`), in this process: `panel` (column-major, its row count is the leading dimension: rows below
    (T - g0) * 128 are never read) against the rank's whole local storage `Cm` (column-major, likewise).  Returns the storage."""
    panel = np.asfortranarray(panel, dtype=np.double)
    Cm = np.asfortranarray(Cm, dtype=np.double).copy(order="F")
    if panel.shape[1] != k:
        raise ValueError("test_gemm_cyc: the panel must have k columns")
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_gemm_cyc(ctx._h, grid[0], grid[1], rank[0], rank[1], nbt, T, row_lo, col_lo, col_hi, g0, k, tri, occ3, alpha, beta,
                                 panel.ctypes.data_as(pd), panel.shape[0], Cm.ctypes.data_as(pd), Cm.shape[0]), "lpgp_test_gemm_cyc")
    return Cm


def test_tile_step(ctx: Context, which: int, XV: np.ndarray, L: np.ndarray, Linv: np.ndarray):
    """In-place refined tile solve on host buffers (`lpgp_test_tile_step`): which = 0: X (rows x 128) <- X L^{-T},
    which = 1: V (128 x cols) <- L^{-1} V.  Returns (result, milliseconds)."""
    XV = np.asfortranarray(XV, dtype=np.double).copy(order="F")
    L = np.asfortranarray(np.tril(L), dtype=np.double)
    Linv = np.asfortranarray(np.tril(Linv), dtype=np.double)
    n = XV.shape[0] if which == 0 else XV.shape[1]
    ms = C.c_double(0.0)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_tile_step(ctx._h, which, XV.ctypes.data_as(pd), n, L.ctypes.data_as(pd), Linv.ctypes.data_as(pd),
                                  C.byref(ms)), "lpgp_test_tile_step")
    return XV, ms.value


def test_panel_solve(ctx: Context, V: np.ndarray, Lblk: np.ndarray, rows_form: bool = False):
    """Fused panel chain (`lpgp_test_panel_solve`): V (nt*128 x cols) <- Lblk^{-1} V, or with `rows_form`
    X (cols x nt*128) <- X Lblk^{-T}.  Returns (result, milliseconds)."""
    if rows_form:
        cols, rows = V.shape
    else:
        rows, cols = V.shape
    nt = rows // 128
    V = np.asfortranarray(V, dtype=np.double).copy(order="F")
    Lb = np.asfortranarray(np.tril(Lblk), dtype=np.double)
    Linv = np.concatenate([np.asfortranarray(np.tril(scipy.linalg.solve_triangular(
        Lb[t * 128:(t + 1) * 128, t * 128:(t + 1) * 128], np.eye(128), lower=True))).reshape(-1, order="F") for t in range(nt)])
    ms = C.c_double(0.0)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_panel_solve(ctx._h, int(bool(rows_form)), V.ctypes.data_as(pd), nt, cols, Lb.ctypes.data_as(pd),
                                    np.ascontiguousarray(Linv).ctypes.data_as(pd), C.byref(ms)), "lpgp_test_panel_solve")
    return V, ms.value


def test_potrf_tile(ctx: Context, T: np.ndarray):
    T = np.asfortranarray(T, dtype=np.double).copy(order="F")
    Linv = np.zeros((128, 128), order="F")
    info = C.c_int32()
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_potrf_tile(ctx._h, T.ctypes.data_as(pd), Linv.ctypes.data_as(pd), C.byref(info)),
          "lpgp_test_potrf_tile")
    return T, Linv, info.value


def solve_vec_fwd(ctx: Context, mat, r: np.ndarray) -> np.ndarray:
    """z = L^{-1} r by the forward half of the single-vector solve as `lpgp_mat_evidence` runs it (`lpgp_test_solve_vec_fwd`; the
    option trsv_resident selects the form).  `r` in Gram order; z comes back in the PADDED layout (`mat.padded_n` doubles)."""
    r = np.ascontiguousarray(r, dtype=np.double)
    if r.shape != (mat.n,):
        raise ValueError(f"residual must have shape ({mat.n},), got {r.shape}")
    z = np.full(mat.padded_n, np.nan)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_solve_vec_fwd(ctx._h, mat._h, r.ctypes.data_as(pd), z.ctypes.data_as(pd)), "lpgp_test_solve_vec_fwd")
    return z


def solve_vec_bwd(ctx: Context, mat, y: np.ndarray) -> np.ndarray:
    """x = L^{-T} y by the backward half of the single-vector solve as `solve_weights` runs it (`lpgp_test_solve_vec_bwd`; the option
    trsv_resident selects the form).  `y` and x in the PADDED layout (`mat.padded_n` doubles); the padding of `y` is taken as given."""
    y = np.ascontiguousarray(y, dtype=np.double)
    if y.shape != (mat.padded_n,):
        raise ValueError(f"right-hand side must have shape ({mat.padded_n},), got {y.shape}")
    x = np.full(mat.padded_n, np.nan)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_solve_vec_bwd(ctx._h, mat._h, y.ctypes.data_as(pd), x.ctypes.data_as(pd)), "lpgp_test_solve_vec_bwd")
    return x


def trsm_lower_t(ctx: Context, mat, V: np.ndarray) -> np.ndarray:
    """L^{-T} V by the multi-column backward substitution of `potrs` alone (`lpgp_test_trsm_lower_t`).  `V`: `mat.padded_n` rows
    (PADDED layout) x a multiple of 128 columns; returns a new column-major array."""
    V = np.array(V, dtype=np.double, order="F")
    if V.ndim != 2 or V.shape[0] != mat.padded_n or V.shape[1] == 0 or V.shape[1] % 128:
        raise ValueError(f"block must have {mat.padded_n} rows and a multiple of 128 columns, got {V.shape}")
    check(lib.lpgp_test_trsm_lower_t(ctx._h, mat._h, V.ctypes.data_as(C.POINTER(C.c_double)), V.shape[1]), "lpgp_test_trsm_lower_t")
    return V


def force_status(ctx: Context, mat, value: int) -> None:
    """Leave the status word of `mat` (a `_engine.GramMatrix`) as an enqueued factorisation ending with `value` would."""
    check(lib.lpgp_test_force_status(ctx._h, mat._h, int(value)), "lpgp_test_force_status")


def set_pool_fill(ctx: Context, byte: int) -> "tuple[int, int]":
    """`lpgp_test_pool_fill`: byte 0..255 switches the fill mode of the device pool on (every buffer handed out is first filled with
    that byte on the panel stream), -1 off (and frees the cached buffers).  Returns (buffers, bytes) filled since the last call."""
    filled = (C.c_int64 * 2)(0, 0)
    check(lib.lpgp_test_pool_fill(ctx._h, int(byte), filled), "lpgp_test_pool_fill")
    return int(filled[0]), int(filled[1])


@contextlib.contextmanager
def pool_fill(ctx: Context, byte: int):
    """The fill mode on with `byte` inside the block, always off behind it.  Yields take(): the (buffers, bytes) filled since the
    last take (or since the mode went on)."""
    set_pool_fill(ctx, byte)
    try:
        yield lambda: set_pool_fill(ctx, byte)
    finally:
        set_pool_fill(ctx, -1)


def mat_raw(ctx: Context, mat, values: np.ndarray | None = None) -> np.ndarray:
    """The padded storage of a matrix (`lpgp_test_mat_raw`): `mat.padded_n` squared, element (r, c) at [r, c], padding rows and the
    part above the diagonal included; `values`: overwrite it with them (and return them)."""
    pn = mat.padded_n
    if values is not None and np.shape(values) != (pn, pn):
        raise ValueError(f"storage must have shape ({pn}, {pn}), got {np.shape(values)}")
    buf = np.empty((pn, pn)) if values is None else np.ascontiguousarray(np.asarray(values).T, dtype=np.double)      # column-major on the device
    check(lib.lpgp_test_mat_raw(ctx._h, mat._h, 0 if values is None else 1, buf.ctypes.data_as(C.POINTER(C.c_double))), "lpgp_test_mat_raw")
    return buf.T


def _vector(mat, v, what: str) -> np.ndarray:
    v = np.ascontiguousarray(v, dtype=np.double)
    if v.shape != (mat.n,):
        raise ValueError(f"{what} must have shape ({mat.n},), got {v.shape}")
    return v


def factor_matmul(ctx: Context, mat, Z: np.ndarray, shift: np.ndarray | None, kc: int) -> np.ndarray:
    """`mat.factor_matmul(Z, shift)` with chunks of `kc` (1, 2, 4 or 8) tiles of columns per workgroup (`lpgp_test_factor_matmul`)
    instead of the chunk size the device would choose."""
    Z = np.ascontiguousarray(Z, dtype=np.double)
    if Z.ndim != 2 or Z.shape[0] != mat.n or Z.shape[1] == 0:
        raise ValueError(f"shape mismatch: factor of order {mat.n} @ {Z.shape}")
    if shift is not None:
        shift = _vector(mat, shift, "shift")
    out = np.full((mat.n, Z.shape[1]), np.nan)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_factor_matmul(ctx._h, mat._h, Z.ctypes.data_as(pd), Z.shape[1], shift.ctypes.data_as(pd) if shift is not None else None,
                                      out.ctypes.data_as(pd), int(kc)), "lpgp_test_factor_matmul")
    return out


def evidence(ctx: Context, mat, r: np.ndarray, max_wgs: int = 0) -> "tuple[float, float]":
    """`mat.evidence(r)` with at most `max_wgs` workgroups in the first stage of the reduction (`lpgp_test_evidence`; 0: as the
    public call)."""
    r = _vector(mat, r, "residual")
    out = np.full(2, np.nan)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_evidence(ctx._h, mat._h, r.ctypes.data_as(pd), int(max_wgs), out.ctypes.data_as(pd)), "lpgp_test_evidence")
    return float(out[0]), float(out[1])


def loo(ctx: Context, mat, r: np.ndarray, y: np.ndarray, max_wgs: int = 0):
    """`mat.loo(r, y)` with at most `max_wgs` workgroups in the epilogue (`lpgp_test_loo`; 0: as the public call)."""
    r, y = _vector(mat, r, "residual"), _vector(mat, y, "observations")
    n = mat.n
    mean, var, logp = np.full(n, np.nan), np.full(n, np.nan), np.full(n + 1, np.nan)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_loo(ctx._h, mat._h, r.ctypes.data_as(pd), y.ctypes.data_as(pd), int(max_wgs), mean.ctypes.data_as(pd), var.ctypes.data_as(pd),
                            logp.ctypes.data_as(pd)), "lpgp_test_loo")
    return mean, var, logp[:n].copy(), float(logp[n])


def evidence_grad(ctx: Context, mat, ginv, dG, r: np.ndarray, max_wgs: int = 0) -> "tuple[float, float]":
    """`mat.evidence_grad(ginv, dG, r)` with at most `max_wgs` workgroups in the contraction (`lpgp_test_evidence_grad`; 0: as the
    public call)."""
    r = _vector(mat, r, "residual")
    out = np.full(2, np.nan)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_evidence_grad(ctx._h, mat._h, ginv._h, dG._h, r.ctypes.data_as(pd), int(max_wgs), out.ctypes.data_as(pd)), "lpgp_test_evidence_grad")
    return float(out[0]), float(out[1])


def evidence_grad_diag(ctx: Context, mat, ginv, bi: int, r: np.ndarray, v: np.ndarray | None = None, scalar: float = 0.0,
                       max_wgs: int = 0) -> "tuple[float, float]":
    """`mat.evidence_grad_diag(ginv, bi, r, v, scalar)` with at most `max_wgs` workgroups (`lpgp_test_evidence_grad_diag`)."""
    r = _vector(mat, r, "residual")
    if v is not None:
        v = np.ascontiguousarray(v, dtype=np.double)
        if v.shape != (mat.block_sizes[bi],):
            raise ValueError("diagonal has the wrong length")
    out = np.full(2, np.nan)
    pd = C.POINTER(C.c_double)
    check(lib.lpgp_test_evidence_grad_diag(ctx._h, mat._h, ginv._h, int(bi), v.ctypes.data_as(pd) if v is not None else None, float(scalar),
                                           r.ctypes.data_as(pd), int(max_wgs), out.ctypes.data_as(pd)), "lpgp_test_evidence_grad_diag")
    return float(out[0]), float(out[1])
