/*
 * lpgp_test.h -- test hooks of the MI355X GP-posterior path.  NOT part of the product ABI (include/lpgp.h):
 * implemented in csrc/testhooks.hip, built into liblpgp_testhooks.so (which links against liblpgp.so) and loaded only
 * by tests/ (tests/_hooks.py) and scratch/.  Raw kernels on host buffers for unit tests and micro-benchmarks, the peak
 * probes, the host replay of the distributed tile enumeration.
 */
#ifndef LPGP_TEST_H
#define LPGP_TEST_H

#include "lpgp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HOST replay of the tile enumeration of a distributed trailing update (no GPU needed): the local tiles of rank
 * (my_r, my_c) of a pr x pc grid in rows [row_lo, T) x columns [col_lo, T) (GLOBAL tile indices, blocks of nbt tiles)
 * that lie on or below the diagonal, in launch order.  out (capacity cap pairs): (global tile row, global tile column)
 * per list entry; returns the number of tiles (< 0: error).                                          */
int  lpgp_test_stair_enumerate(int32_t pr, int32_t pc, int32_t my_r, int32_t my_c, int32_t nbt, int32_t T,
                               int32_t row_lo, int32_t col_lo, int32_t* out, int64_t cap);
/* The distributed trailing update of ONE rank, in this process, on host buffers: rank (my_r, my_c) of a pr x pc grid (blocks of nbt
 * tiles, T tile rows / columns in all) updates its local tiles whose global tile (gr, gc) has gr >= row_lo, col_lo <= gc < col_hi and
 * gr >= gc:  C <- beta C + alpha P[gr - g0] P[gc - g0]^T.  The launch arguments come from the function the factorisation itself uses
 * (update_args, csrc/dist.hip) and go through launch_gemm.  panel: rows of the global tiles g0 .. T - 1 (g0 <= row_lo, col_lo), k columns
 * (a multiple of 128), column-major, leading dimension ldp >= (T - g0) * 128.  C: the rank's WHOLE local storage, cyc_before(rows, T) x
 * cyc_before(cols, T) tiles, column-major, leading dimension ldc.  tri: 1 (remainder / whole update) or 3 (look-ahead half); occ3: the
 * launch may use the three-workgroups-per-CU kernel.  A rank that owns nothing of the region returns 0 and touches nothing.         */
int  lpgp_test_gemm_cyc(lpgp_ctx* ctx, int32_t pr, int32_t pc, int32_t my_r, int32_t my_c, int32_t nbt, int32_t T, int32_t row_lo,
                        int32_t col_lo, int32_t col_hi, int32_t g0, int32_t k, int32_t tri, int32_t occ3, double alpha, double beta,
                        const double* panel, int64_t ldp, double* C, int64_t ldc);
/* C(m x n, col-major ldc) = beta*C + alpha * op(A) op(B); ta/tb: 0 => operand stored with
 * its non-contracted index fastest, 1 => contracted index (k) fastest.                  */
int  lpgp_test_gemm(lpgp_ctx* ctx, int32_t ta, int32_t tb, int32_t lower_only,
                    int64_t m, int64_t n, int64_t k, double alpha,
                    const double* A, int64_t lda, const double* B, int64_t ldb,
                    double beta, double* C, int64_t ldc, int32_t reps, double* ms_per_rep);
/* in-place 128x128 tile Cholesky + inverse: T (col-major 128x128) -> L, Linv            */
int  lpgp_test_potrf_tile(lpgp_ctx* ctx, double* T, double* Linv, int32_t* info);
/* the two in-place tile solves of the panel chain / forward substitution on host buffers, each with its one
 * step of iterative refinement (X0 = A Linv^T, X = X0 + (A - X0 L^T) Linv^T):
 *   which = 0:  X (rows x 128, col-major ldx = rows, rows a multiple of 128) <- X * L^{-T}
 *   which = 1:  V (128 x cols, col-major ld 128, cols a multiple of 128) <- L^{-1} * V
 * L, Linv: 128 x 128 column-major, lower triangular WITH ZEROS above the diagonal (as the tile Cholesky
 * stores them); Linv the fp64 inverse of L.                                                    */
int  lpgp_test_tile_step(lpgp_ctx* ctx, int32_t which, double* XV, int64_t n, const double* L,
                         const double* Linv, double* ms);
/* the fused panel step of the forward substitution on host buffers: V (nt * 128 rows x cols, col-major, ld = nt * 128,
 * cols a multiple of 128) <- Lblk^{-1} V with Lblk the nt x nt tile lower-triangular block (col-major, ld nt * 128, the
 * diagonal TILES with zeros above their diagonal) and Linv the nt explicit inverses of its diagonal tiles.
 * rows_form != 0: the same chain for rows, X (cols rows x nt * 128 columns, col-major, ld = cols) <- X Lblk^{-T}
 * (the panel solve of the multi-GPU factorisation and of a block append).                                       */
int  lpgp_test_panel_solve(lpgp_ctx* ctx, int32_t rows_form, double* V, int32_t nt, int64_t cols, const double* Lblk,
                           const double* Linv, double* ms);
/* diagnostics: histogram over the 8 XCDs of where the single workgroup of the tile Cholesky ran
 * since the last reset (the CU reservation of the update streams is built on it)           */
int  lpgp_debug_tile_xcc(lpgp_ctx* ctx, int32_t* out8, int32_t reset);
/* peak probes: fp64 MFMA issue loop and streaming write; returns TFLOP/s resp. GB/s     */
int  lpgp_probe_mfma_f64(lpgp_ctx* ctx, double* tflops);
int  lpgp_probe_hbm_write(lpgp_ctx* ctx, int64_t bytes, double* gbps);

/* leaves the sticky status word of `mat` as an enqueued factorisation that ended with `value` would (value < 0: a hand-over of
 * a resident kernel timed out): the error path of lpgp_mat_check without a broken device                          */
int  lpgp_test_force_status(lpgp_ctx* ctx, lpgp_mat* mat, int32_t value);

/* Fill mode of the device pool: the library never clears a buffer it hands out ("What a buffer holds"), and this makes
 * every result's independence of stale storage testable.  byte in 0..255: from now on every buffer the pool hands out, cached or
 * fresh, and every (re)allocation of the persistent scratch is first filled with that byte, enqueued on the panel stream; the scratch
 * the context holds now is filled at once.  byte == -1: off (the default); the device is waited for and every cached pool buffer is
 * freed, so that later work starts from fresh allocations as it does without the hook.  filled (may be NULL): the buffers and
 * bytes filled since the last call, which resets them.  Refused: a context of a multi-GPU job, any other value of byte.  */
int  lpgp_test_pool_fill(lpgp_ctx* ctx, int32_t byte, int64_t filled[2]);

/* the forward half of the single-vector solve alone, z = L^{-1} r, as lpgp_mat_evidence runs it: r_host (logical order,
 * lpgp_mat_size doubles) is staged into the padded layout with zeros in the padding rows, solved by the form the option
 * trsv_resident selects (1: the resident kernel of trsv.hip, 0: one launch per tile row, potrf.hip), and z comes back in the
 * PADDED layout (lpgp_mat_padded_size doubles).  A negative status word (a timed-out hand-over) is returned as an error.  */
int  lpgp_test_solve_vec_fwd(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, double* z_host_padded);
/* the backward half of the single-vector solve alone, x = L^{-T} y, by the functions lpgp_solve_weights, lpgp_mat_loo, lpgp_mat_cv and
 * the evidence gradients run it through (the form the option trsv_resident selects).  y and x are in the PADDED layout
 * (lpgp_mat_padded_size doubles each); y is taken as given, padding entries included.  Same refusals and status handling as above. */
int  lpgp_test_solve_vec_bwd(lpgp_ctx* ctx, lpgp_mat* mat, const double* y_host_padded, double* x_host_padded);
/* the multi-column backward substitution of lpgp_potrs alone (trsm_lower_t_blocked), V <- L^{-T} V in place on a host block of
 * lpgp_mat_padded_size rows x m_pad columns, column-major with the padded size as leading dimension; m_pad a multiple of 128.
 * Single GPU, fully factored, status read.                                                                          */
int  lpgp_test_trsm_lower_t(lpgp_ctx* ctx, lpgp_mat* mat, double* v_host_padded, int64_t m_pad);

/* the raw storage of the view of `mat` -- lpgp_mat_padded_size squared doubles, column-major, leading dimension the padded size, the
 * padding rows and the tiles above the diagonal included -- read into `host` (set == 0) or overwritten from it (set != 0): what the
 * padded layout holds, and operands no assembly produces (garbage in the padding, a chosen lower triangle under a factored state).
 * Single GPU; the state of `mat` (factored or not) is left as it is.                                                  */
int  lpgp_test_mat_raw(lpgp_ctx* ctx, lpgp_mat* mat, int32_t set, double* host);

/* lpgp_mat_factor_matmul with the chunk size of its first kernel given: kc = 1, 2, 4 or 8 tiles of columns per workgroup, instead
 * of the one the size and the CU count choose.  Every kc computes the same product.  Refuses what the public call refuses.   */
int  lpgp_test_factor_matmul(lpgp_ctx* ctx, lpgp_mat* mat, const double* Z_host, int64_t s, const double* shift_host,
                             double* out_host, int32_t kc);
/* lpgp_mat_evidence, lpgp_mat_loo, lpgp_mat_evidence_grad and lpgp_mat_evidence_grad_diag with at most max_wgs workgroups in the first
 * stage of their reductions (0: the launch of the public call), so that a thread or a wave takes several rows or columns at a size a
 * test can afford.  Arguments, results and refusals are the public calls'.                                             */
int  lpgp_test_evidence(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, int32_t max_wgs, double out_host[2]);
int  lpgp_test_loo(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, const double* y_host, int32_t max_wgs, double* mean_host,
                   double* var_host, double* logp_host);
int  lpgp_test_evidence_grad(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, const lpgp_mat* dG, const double* r_host,
                             int32_t max_wgs, double out_host[2]);
int  lpgp_test_evidence_grad_diag(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, int32_t bi, const double* v_host, double scalar,
                                  const double* r_host, int32_t max_wgs, double out_host[2]);

#ifdef __cplusplus
}
#endif
#endif /* LPGP_TEST_H */
