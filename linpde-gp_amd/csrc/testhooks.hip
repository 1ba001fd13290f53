// Test hooks of liblpgp.so -- NOT part of the product.  Built into a library of its own (`liblpgp_testhooks.so`, build.sh),
// which links against liblpgp.so and is loaded only by tests/ and scratch/ (tests/_hooks.py): raw kernels on host buffers for
// unit tests and micro-benchmarks, the peak probes, and the host replay of the distributed tile enumeration.  Declared in
// include/lpgp_test.h.  `nm -D liblpgp.so | grep -E "lpgp_(test|probe|debug)"` is empty.

#include <cstdlib>
#include <cstring>
#include <vector>

#include "lpgp_internal.h"
#include "lpgp_test.h"

namespace lpgp {

typedef double v4f64 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void mfma_probe_kernel(double* out, int iters) {
  v4f64 acc[8];
  const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = (v4f64){0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[blockIdx.x * (int64_t)blockDim.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void write_probe_kernel(double* out, int64_t n2) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n2; i += stride)
    reinterpret_cast<double2*>(out)[i] = make_double2((double)i, 1.0);
}

}  // namespace lpgp

using namespace lpgp;

extern "C" {

// ---- raw kernels for unit tests / microbenchmarks ---------------------------------------------
int lpgp_test_gemm(lpgp_ctx* ctx, int32_t ta, int32_t tb, int32_t lower_only, int64_t m, int64_t n, int64_t k,
                   double alpha, const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                   double* C, int64_t ldc, int32_t reps, double* ms_per_rep) {
  LPGP_DEVICE(ctx);
  hipStream_t ts = ctx->s_main;
  if (const char* e = std::getenv("LPGP_TEST_GEMM_STREAM")) { const int v = std::atoi(e); ts = v == 1 ? ctx->s_upd : (v == 2 && ctx->s_upd_narrow ? ctx->s_upd_narrow : ctx->s_main); }
  LPGP_CHECK(m % TILE == 0 && n % TILE == 0 && k % 16 == 0, "lpgp_test_gemm: m,n multiples of 128 and k of 16 required");
  const int64_t a_elems = ta ? lda * m : lda * k;
  const int64_t b_elems = tb ? ldb * n : ldb * k;
  DevBuf bA, bB, bC;
  LPGP_TRY(DevBuf::raw((size_t)a_elems * sizeof(double), &bA));
  LPGP_TRY(DevBuf::raw((size_t)b_elems * sizeof(double), &bB));
  LPGP_TRY(DevBuf::raw((size_t)ldc * n * sizeof(double), &bC));
  double *const dA = bA.as(), *const dB = bB.as(), *const dC = bC.as();
  LPGP_HIP(hipMemcpy(dA, A, (size_t)a_elems * sizeof(double), hipMemcpyHostToDevice));
  LPGP_HIP(hipMemcpy(dB, B, (size_t)b_elems * sizeof(double), hipMemcpyHostToDevice));
  LPGP_HIP(hipMemcpy(dC, C, (size_t)ldc * n * sizeof(double), hipMemcpyHostToDevice));
  GemmArgs g;
  g.A = dA; g.B = dB; g.C = dC; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.mt = (int)(m / TILE); g.nt = (int)(n / TILE); g.k = (int)k; g.alpha = alpha; g.beta = beta;
  g.tri = lower_only;
  LPGP_TRY(launch_gemm(ctx, ts, ta, tb, g, -1));
  LPGP_HIP(hipStreamSynchronize(ts));
  LPGP_HIP(hipMemcpy(C, dC, (size_t)ldc * n * sizeof(double), hipMemcpyDeviceToHost));
  if (reps > 0 && ms_per_rep) {
    EventPair ev;
    LPGP_TRY(ev.create());
    LPGP_HIP(hipEventRecord(ev.e0, ts));
    for (int r = 0; r < reps; ++r) LPGP_TRY(launch_gemm(ctx, ts, ta, tb, g, -1));
    LPGP_HIP(hipEventRecord(ev.e1, ts));
    LPGP_HIP(hipEventSynchronize(ev.e1));
    float ms = 0.f;
    LPGP_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *ms_per_rep = ms / reps;
  }
  return 0;
}

int lpgp_test_stair_enumerate(int32_t pr, int32_t pc, int32_t my_r, int32_t my_c, int32_t nbt, int32_t T, int32_t row_lo,
                              int32_t col_lo, int32_t* out, int64_t cap) {
  LPGP_CHECK(pr >= 1 && pc >= 1 && my_r >= 0 && my_r < pr && my_c >= 0 && my_c < pc && nbt >= 1 && T >= 0 && out, "lpgp_test_stair_enumerate: bad argument");
  GemmArgs g;
  g.cyc = 1; g.tri = 1;
  g.rowc.P = pr; g.rowc.me = my_r; g.rowc.nbt = nbt;
  g.colc.P = pc; g.colc.me = my_c; g.colc.nbt = nbt;
  g.rt0 = cyc_before(g.rowc, row_lo);
  g.ct0 = cyc_before(g.colc, col_lo);
  g.mt = cyc_before(g.rowc, T) - g.rt0;
  g.nt = cyc_before(g.colc, T) - g.ct0;
  g.g0 = col_lo < row_lo ? col_lo : row_lo;
  if (g.mt <= 0 || g.nt <= 0) return 0;
  const int n = stair_enumerate_host(g, out, cap);
  for (int64_t i = 0; i < n && i < cap; ++i) {      // local -> global tile indices
    out[2 * i] = cyc_l2g(g.rowc, g.rt0 + out[2 * i]);
    out[2 * i + 1] = cyc_l2g(g.colc, g.ct0 + out[2 * i + 1]);
  }
  return n;
}

// The trailing update of rank (my_r, my_c) of a pr x pc grid as potrf_dist launches it, on host buffers: the arguments come from
// update_args (dist.hip), the launch goes through launch_gemm.  Chost: the rank's whole local storage, cyc_before(rows, T) x
// cyc_before(cols, T) tiles (leading dimension ldc); panel: rows of global tiles g0 ... T - 1, k columns (leading dimension ldp).
int lpgp_test_gemm_cyc(lpgp_ctx* ctx, int32_t pr, int32_t pc, int32_t my_r, int32_t my_c, int32_t nbt, int32_t T, int32_t row_lo,
                       int32_t col_lo, int32_t col_hi, int32_t g0, int32_t k, int32_t tri, int32_t occ3, double alpha, double beta,
                       const double* panel, int64_t ldp, double* Chost, int64_t ldc) {
  LPGP_CHECK(ctx && pr >= 1 && pc >= 1 && my_r >= 0 && my_r < pr && my_c >= 0 && my_c < pc && nbt >= 1 && T >= 1,
             "lpgp_test_gemm_cyc: bad grid");
  LPGP_CHECK(row_lo >= 0 && row_lo <= T && col_lo >= 0 && col_lo <= col_hi && col_hi <= T && g0 >= 0 && g0 <= row_lo && g0 <= col_lo,
             "lpgp_test_gemm_cyc: bad region (0 <= g0 <= row_lo, col_lo; col_lo <= col_hi <= T)");
  LPGP_CHECK((tri == 1 || tri == 3) && k > 0 && k % TILE == 0 && alpha != 0.0, "lpgp_test_gemm_cyc: tri is 1 or 3, k a multiple of 128, alpha != 0");
  LPGP_DEVICE(ctx);
  Cyc R, Cc;
  R.P = pr; R.me = my_r; R.nbt = nbt;
  Cc.P = pc; Cc.me = my_c; Cc.nbt = nbt;
  const int LTr = cyc_before(R, T), LTc = cyc_before(Cc, T);
  const int rt0 = cyc_before(R, row_lo), ct0 = cyc_before(Cc, col_lo), ct1 = cyc_before(Cc, col_hi);
  if (LTr == 0 || LTc == 0 || LTr <= rt0 || ct1 <= ct0) return 0;       // nothing of the region on this rank (update_local)
  LPGP_CHECK(panel && Chost && ldp >= (int64_t)(T - g0) * TILE && ldc >= (int64_t)LTr * TILE, "lpgp_test_gemm_cyc: a leading dimension is too small");
  const size_t pbytes = (size_t)ldp * (size_t)k * sizeof(double), cbytes = (size_t)ldc * (size_t)LTc * TILE * sizeof(double);
  DevBuf bP, bC;
  LPGP_TRY(DevBuf::raw(pbytes, &bP));
  LPGP_TRY(DevBuf::raw(cbytes, &bC));
  LPGP_HIP(hipMemcpy(bP.as(), panel, pbytes, hipMemcpyHostToDevice));
  LPGP_HIP(hipMemcpy(bC.as(), Chost, cbytes, hipMemcpyHostToDevice));
  GemmArgs g = update_args(bC.as(), ldc, R, Cc, bP.as(), ldp, g0, k, rt0, LTr, ct0, ct1, tri);
  g.alpha = alpha; g.beta = beta; g.occ3 = occ3;
  LPGP_TRY(launch_gemm(ctx, ctx->s_main, 0, 0, g, -1));
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));
  LPGP_HIP(hipMemcpy(Chost, bC.as(), cbytes, hipMemcpyDeviceToHost));
  return 0;
}

int lpgp_test_potrf_tile(lpgp_ctx* ctx, double* T, double* Linv, int32_t* info) {
  LPGP_DEVICE(ctx);
  const size_t tbytes = (size_t)TILE * TILE * sizeof(double);
  int h = 0;
  if (info) *info = h;
  DevBuf bT, bL;                                 // (hipFree waits for the device: h, declared in front, outlives a copy in flight)
  LPGP_TRY(DevBuf::raw(tbytes, &bT));
  LPGP_TRY(DevBuf::raw(tbytes, &bL));
  double *const dT = bT.as(), *const dL = bL.as();
  LPGP_HIP(hipMemcpy(dT, T, tbytes, hipMemcpyHostToDevice));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), ctx->s_main));
  LPGP_TRY(launch_potrf_tile(ctx, ctx->s_main, dT, TILE, dL, ctx->d_info, 0, TileForm::plain));
  LPGP_HIP(hipMemcpyAsync(&h, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, ctx->s_main));
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));
  LPGP_HIP(hipMemcpy(T, dT, tbytes, hipMemcpyDeviceToHost));
  LPGP_HIP(hipMemcpy(Linv, dL, tbytes, hipMemcpyDeviceToHost));
  if (info) *info = h;
  return 0;
}

int lpgp_test_tile_step(lpgp_ctx* ctx, int32_t which, double* XV, int64_t n, const double* L, const double* Linv, double* ms) {
  LPGP_CHECK(ctx && XV && L && Linv && n > 0 && n % TILE == 0 && (which == 0 || which == 1), "lpgp_test_tile_step: bad argument");
  LPGP_DEVICE(ctx);
  const size_t bytes = (size_t)n * TILE * sizeof(double), tbytes = (size_t)TILE * TILE * sizeof(double);
  DevBuf bd, bl, bt;
  LPGP_TRY(DevBuf::raw(bytes, &bd));
  LPGP_TRY(DevBuf::raw(tbytes, &bl));
  LPGP_TRY(DevBuf::raw(tbytes, &bt));
  double *const d = bd.as(), *const dl = bl.as(), *const dt = bt.as();
  LPGP_HIP(hipMemcpy(d, XV, bytes, hipMemcpyHostToDevice));
  LPGP_HIP(hipMemcpy(dl, Linv, tbytes, hipMemcpyHostToDevice));
  LPGP_HIP(hipMemcpy(dt, L, tbytes, hipMemcpyHostToDevice));
  EventPair ev;
  LPGP_TRY(ev.create());
  const int nt = (int)(n / TILE);
  LPGP_HIP(hipEventRecord(ev.e0, ctx->s_main));
  LPGP_TRY(which == 0 ? launch_trsm_tile(ctx, ctx->s_main, d, n, dl, dt, TILE, nt, -1)
                      : launch_trsv_tile(ctx, ctx->s_main, d, TILE, dl, dt, TILE, nt, -1));
  LPGP_HIP(hipEventRecord(ev.e1, ctx->s_main));
  LPGP_HIP(hipEventSynchronize(ev.e1));
  float t = 0.f;
  LPGP_HIP(hipEventElapsedTime(&t, ev.e0, ev.e1));
  if (ms) *ms = t;
  LPGP_HIP(hipMemcpy(XV, d, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int lpgp_test_panel_solve(lpgp_ctx* ctx, int32_t rows_form, double* V, int32_t nt, int64_t cols, const double* Lblk, const double* Linv, double* ms) {
  LPGP_CHECK(ctx && V && Lblk && Linv && nt >= 1 && nt <= 4 && cols > 0 && cols % TILE == 0, "lpgp_test_panel_solve: bad argument");
  LPGP_DEVICE(ctx);
  const int64_t rows = (int64_t)nt * TILE;
  const size_t vb = (size_t)rows * cols * sizeof(double), lb = (size_t)rows * rows * sizeof(double), ib = (size_t)nt * TILE * TILE * sizeof(double);
  DevBuf bd, bl, bi;
  LPGP_TRY(DevBuf::raw(vb, &bd));
  LPGP_TRY(DevBuf::raw(lb, &bl));
  LPGP_TRY(DevBuf::raw(ib, &bi));
  double *const d = bd.as(), *const dl = bl.as(), *const di = bi.as();
  LPGP_HIP(hipMemcpy(d, V, vb, hipMemcpyHostToDevice));
  LPGP_HIP(hipMemcpy(dl, Lblk, lb, hipMemcpyHostToDevice));
  LPGP_HIP(hipMemcpy(di, Linv, ib, hipMemcpyHostToDevice));
  EventPair ev;
  LPGP_TRY(ev.create());
  LPGP_HIP(hipEventRecord(ev.e0, ctx->s_main));
  // rows_form: V holds X (cols rows x nt * 128 columns, column-major ld = cols) and X <- X Lblk^{-T}
  LPGP_TRY(rows_form ? launch_trsm_panel(ctx, ctx->s_main, d, cols, di, dl, rows, nt, (int)(cols / TILE), -1)
                     : launch_trsv_panel(ctx, ctx->s_main, d, rows, di, dl, rows, nt, (int)(cols / TILE), -1));
  LPGP_HIP(hipEventRecord(ev.e1, ctx->s_main));
  LPGP_HIP(hipEventSynchronize(ev.e1));
  float t = 0.f;
  LPGP_HIP(hipEventElapsedTime(&t, ev.e0, ev.e1));
  if (ms) *ms = t;
  LPGP_HIP(hipMemcpy(V, d, vb, hipMemcpyDeviceToHost));
  return 0;
}

int lpgp_debug_tile_xcc(lpgp_ctx* ctx, int32_t* out8, int32_t reset) {
  LPGP_CHECK(ctx && out8, "lpgp_debug_tile_xcc: null argument");
  LPGP_DEVICE(ctx);
  LPGP_HIP(hipDeviceSynchronize());
  return debug_tile_xcc(out8, reset);
}

int lpgp_probe_mfma_f64(lpgp_ctx* ctx, double* tflops) {
  LPGP_DEVICE(ctx);
  const int blocks = ctx->cus * 4, iters = 4000;
  DevBuf buf;
  LPGP_TRY(DevBuf::raw((size_t)blocks * 256 * sizeof(double), &buf));
  double* const d = buf.as();
  EventPair ev;
  LPGP_TRY(ev.create());
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(blocks), dim3(256), 0, ctx->s_main, d, 100);   // warm-up
  LPGP_HIP(hipEventRecord(ev.e0, ctx->s_main));
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(blocks), dim3(256), 0, ctx->s_main, d, iters);
  LPGP_HIP(hipEventRecord(ev.e1, ctx->s_main));
  LPGP_HIP(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  LPGP_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  const double flops = (double)blocks * 4.0 * iters * 8.0 * (2.0 * 16 * 16 * 4);
  if (tflops) *tflops = flops / (ms * 1e-3) / 1e12;
  return 0;
}

int lpgp_probe_hbm_write(lpgp_ctx* ctx, int64_t bytes, double* gbps) {
  LPGP_DEVICE(ctx);
  bytes = round_up(bytes, 16);
  DevBuf buf;
  LPGP_TRY(DevBuf::raw((size_t)bytes, &buf));
  double* const d = buf.as();
  EventPair ev;
  LPGP_TRY(ev.create());
  const int grid = ctx->cus * 8;
  hipLaunchKernelGGL(write_probe_kernel, dim3(grid), dim3(256), 0, ctx->s_main, d, bytes / 16);
  LPGP_HIP(hipEventRecord(ev.e0, ctx->s_main));
  for (int r = 0; r < 5; ++r)
    hipLaunchKernelGGL(write_probe_kernel, dim3(grid), dim3(256), 0, ctx->s_main, d, bytes / 16);
  LPGP_HIP(hipEventRecord(ev.e1, ctx->s_main));
  LPGP_HIP(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  LPGP_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  if (gbps) *gbps = 5.0 * (double)bytes / (ms * 1e-3) / 1e9;
  return 0;
}

// the status word of `mat` as an enqueued factorisation that ended with `value` would leave it (value < 0: a timed-out hand-over)
int lpgp_test_force_status(lpgp_ctx* ctx, lpgp_mat* mat, int32_t value) {
  LPGP_CHECK(ctx && mat, "lpgp_test_force_status: null argument");
  LPGP_DEVICE(ctx);
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));
  LPGP_HIP(hipMemcpy(mat->d_status, &value, sizeof(int), hipMemcpyHostToDevice));
  mat->status_pending();
  return 0;
}

// The fill mode of the device pool (ctx->pool_fill, api.hip pool_alloc / ensure_tmp).  byte 0..255: on, and the persistent scratch is
// filled at once; -1: off, the device waited for and every cached pool buffer freed, so that what runs next starts from fresh
// allocations as it does without the hook.  filled (may be NULL): buffers and bytes filled since the last call, then reset.
int lpgp_test_pool_fill(lpgp_ctx* ctx, int32_t byte, int64_t filled[2]) {
  LPGP_CHECK(byte >= -1 && byte <= 255, "lpgp_test_pool_fill: the fill is a byte (0..255) or -1 (off), not %d", byte);
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "lpgp_test_pool_fill: single GPU only");
  if (byte >= 0) {
    ctx->pool_fill = byte;
    if (ctx->d_tmp && ctx->tmp_cap > 0) {
      LPGP_HIP(hipMemsetAsync(ctx->d_tmp, byte, (size_t)ctx->tmp_cap * sizeof(double), ctx->s_main));
      ctx->pool_filled[0] += 1;
      ctx->pool_filled[1] += ctx->tmp_cap * (int64_t)sizeof(double);
    }
  } else {
    ctx->pool_fill = -1;
    LPGP_HIP(hipDeviceSynchronize());
    for (auto& b : ctx->pool) (void)hipFree(b.p);
    ctx->pool.clear();
  }
  if (filled) {
    filled[0] = ctx->pool_filled[0];
    filled[1] = ctx->pool_filled[1];
  }
  ctx->pool_filled[0] = ctx->pool_filled[1] = 0;
  return 0;
}

// the refusals the hooks on a factor share: single GPU, fully factored, status read
#define LPGP_TEST_FACTORED(ctx, mat, who)                                                                                          \
  do {                                                                                                                             \
    LPGP_MAT_ALIVE(mat, who);                                                                                                      \
    LPGP_CHECK(!(ctx)->distributed(), who ": single GPU only");                                                                    \
    LPGP_CHECK((mat)->pn > 0 && (mat)->pn_fact == (mat)->pn, who ": matrix is not (fully) factored");                              \
    LPGP_CHECK(!(mat)->unchecked, who ": the status of an enqueued factorisation has not been read (lpgp_mat_check)");             \
  } while (0)

// z = L^{-1} r, the forward half of the single-vector solve alone, as lpgp_mat_evidence runs it: r scattered into the padded layout
// (zeros in the padding rows), the dispatch on ctx->trsv_resident (trsv.hip solve_vec_fwd_resident, else potrf.hip solve_vec_fwd),
// z back in the padded layout (mat->pn doubles).  A negative status word (a timed-out hand-over) is a library error.
int lpgp_test_solve_vec_fwd(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, double* z_host_padded) {
  LPGP_CHECK(ctx && mat && r_host && z_host_padded, "lpgp_test_solve_vec_fwd: null argument");
  LPGP_DEVICE(ctx);
  LPGP_TEST_FACTORED(ctx, mat, "lpgp_test_solve_vec_fwd");
  const int64_t pn = mat->pn, T = pn / TILE;
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  std::vector<double> h((size_t)pn);
  int info = 0;
  mat->scatter_padded(r_host, h.data());
  // [r as staged | z + the ticket word of the resident solve]
  DevBuf buf;
  LPGP_TRY(DevBuf::raw((size_t)(2 * pn + 2) * sizeof(double), &buf));
  double* const d = buf.as();
  StreamDrain drain{st};                         // (the staging vector, the status word and the caller's array are borrowed by the copies)
  LPGP_HIP(hipMemcpyAsync(d, h.data(), (size_t)pn * sizeof(double), hipMemcpyHostToDevice, st));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  if (ctx->trsv_resident) LPGP_TRY(solve_vec_fwd_resident(ctx, F, T, d, d + pn, ctx->d_info));
  else LPGP_TRY(solve_vec_fwd(ctx, st, F, T, d, d + pn));
  LPGP_HIP(hipMemcpyAsync(z_host_padded, d + pn, (size_t)pn * sizeof(double), hipMemcpyDeviceToHost, st));
  LPGP_HIP(hipMemcpyAsync(&info, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, st));
  LPGP_TRY(drain.wait());
  LPGP_CHECK(info >= 0, "lpgp_test_solve_vec_fwd: resident single-vector solve: a hand-over between workgroups timed out (status %d)", info);
  return 0;
}

// x = L^{-T} y, the backward half of the single-vector solve alone, by the functions solve_vec / solve_vec_resident call for it
// (potrf.hip solve_vec_bwd, trsv.hip solve_vec_bwd_resident; the dispatch on ctx->trsv_resident is solve_vec's).  y is taken as
// given, padding entries included; both vectors in the padded layout (mat->pn doubles).  A negative status word is a library error.
int lpgp_test_solve_vec_bwd(lpgp_ctx* ctx, lpgp_mat* mat, const double* y_host_padded, double* x_host_padded) {
  LPGP_CHECK(ctx && mat && y_host_padded && x_host_padded, "lpgp_test_solve_vec_bwd: null argument");
  LPGP_DEVICE(ctx);
  LPGP_TEST_FACTORED(ctx, mat, "lpgp_test_solve_vec_bwd");
  const int64_t pn = mat->pn, T = pn / TILE;
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  int info = 0;
  // [x | y + the two ticket words of the resident solve: the backward half counts the second one up from -1]
  DevBuf buf;
  LPGP_TRY(DevBuf::raw((size_t)(2 * pn + 2) * sizeof(double), &buf));
  double *const x = buf.as(), *const y = x + pn;
  StreamDrain drain{st};                         // (the status word and the caller's arrays are borrowed by the copies)
  LPGP_HIP(hipMemcpyAsync(y, y_host_padded, (size_t)pn * sizeof(double), hipMemcpyHostToDevice, st));
  LPGP_HIP(hipMemsetAsync(y + pn, 0xFF, 2 * sizeof(double), st));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  if (ctx->trsv_resident) LPGP_TRY(solve_vec_bwd_resident(ctx, F, T, y, x, ctx->d_info));
  else LPGP_TRY(solve_vec_bwd(ctx, st, F, T, y, x));
  LPGP_HIP(hipMemcpyAsync(x_host_padded, x, (size_t)pn * sizeof(double), hipMemcpyDeviceToHost, st));
  LPGP_HIP(hipMemcpyAsync(&info, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, st));
  LPGP_TRY(drain.wait());
  LPGP_CHECK(info >= 0, "lpgp_test_solve_vec_bwd: resident single-vector solve: a hand-over between workgroups timed out (status %d)", info);
  return 0;
}

// V <- L^{-T} V by trsm_lower_t_blocked alone (the backward half of lpgp_potrs), in place on a host block of pn x m_pad doubles,
// column-major with leading dimension pn, m_pad a multiple of 128; the FactorView is the one solve_lower_t (api.hip) builds.
int lpgp_test_trsm_lower_t(lpgp_ctx* ctx, lpgp_mat* mat, double* v_host, int64_t m_pad) {
  LPGP_CHECK(ctx && mat && v_host && m_pad > 0 && m_pad % TILE == 0, "lpgp_test_trsm_lower_t: bad argument (m_pad a positive multiple of 128)");
  LPGP_DEVICE(ctx);
  LPGP_TEST_FACTORED(ctx, mat, "lpgp_test_trsm_lower_t");
  const int64_t pn = mat->pn;
  const size_t bytes = (size_t)pn * (size_t)m_pad * sizeof(double);
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  DevBuf dv;
  LPGP_TRY(DevBuf::raw(bytes, &dv));
  StreamDrain drain{st};                         // (the caller's array is borrowed by the copies)
  LPGP_HIP(hipMemcpyAsync(dv.as(), v_host, bytes, hipMemcpyHostToDevice, st));
  LPGP_TRY(trsm_lower_t_blocked(ctx, F, pn / TILE, dv.as(), pn, m_pad));
  LPGP_HIP(hipMemcpyAsync(v_host, dv.as(), bytes, hipMemcpyDeviceToHost, st));
  LPGP_TRY(drain.wait());
  return 0;
}

// the raw storage of the view of `mat` -- pn x pn doubles, column-major, leading dimension pn, padding rows and the tiles above the
// diagonal included -- read (set == 0) or overwritten (set != 0): what the padded layout holds, and operands with garbage in the padding.
int lpgp_test_mat_raw(lpgp_ctx* ctx, lpgp_mat* mat, int32_t set, double* host) {
  LPGP_CHECK(ctx && mat && host && mat->pn > 0, "lpgp_test_mat_raw: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "lpgp_test_mat_raw: single GPU only");
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));
  const size_t row = (size_t)mat->pn * sizeof(double), ld = (size_t)mat->lr_cap * sizeof(double);
  if (set) LPGP_HIP(hipMemcpy2D(mat->a, ld, host, row, row, (size_t)mat->pn, hipMemcpyHostToDevice));
  else LPGP_HIP(hipMemcpy2D(host, row, mat->a, ld, row, (size_t)mat->pn, hipMemcpyDeviceToHost));
  return 0;
}

// lpgp_mat_factor_matmul with the chunk size of trmm_lower_kernel given (kc = 1, 2, 4 or 8 tiles of columns per workgroup) instead of
// chosen from the size and the CU count; refuses what the public call refuses
int lpgp_test_factor_matmul(lpgp_ctx* ctx, lpgp_mat* mat, const double* Z_host, int64_t s, const double* shift_host, double* out_host, int32_t kc) {
  LPGP_CHECK(ctx && mat && Z_host && out_host && s >= 1, "lpgp_test_factor_matmul: bad argument");
  LPGP_CHECK(kc == 1 || kc == 2 || kc == 4 || kc == 8, "lpgp_test_factor_matmul: the chunk size is 1, 2, 4 or 8 tiles, not %d", kc);
  LPGP_DEVICE(ctx);
  LPGP_TEST_FACTORED(ctx, mat, "lpgp_test_factor_matmul");
  return factor_matmul(ctx, mat, Z_host, s, shift_host, out_host, kc);
}

// lpgp_mat_evidence / lpgp_mat_loo / lpgp_mat_evidence_grad / lpgp_mat_evidence_grad_diag with at most max_wgs workgroups in the
// stage-1 reduction (max_wgs >= 1; 0: the launch of the public call), so that a thread or a wave takes several rows or columns at a size
// a test can hold a reference for; each refuses what its public call refuses
int lpgp_test_evidence(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, int32_t max_wgs, double out_host[2]) {
  LPGP_CHECK(ctx && mat && r_host && out_host && max_wgs >= 0, "lpgp_test_evidence: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_TEST_FACTORED(ctx, mat, "lpgp_test_evidence");
  return mat_evidence(ctx, mat, r_host, out_host, max_wgs);
}

int lpgp_test_loo(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, const double* y_host, int32_t max_wgs, double* mean_host, double* var_host,
                  double* logp_host) {
  LPGP_CHECK(ctx && mat && r_host && y_host && mean_host && var_host && logp_host && max_wgs >= 0, "lpgp_test_loo: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_TEST_FACTORED(ctx, mat, "lpgp_test_loo");
  return mat_loo(ctx, mat, r_host, y_host, mean_host, var_host, logp_host, max_wgs);
}

int lpgp_test_evidence_grad(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, const lpgp_mat* dG, const double* r_host, int32_t max_wgs,
                            double out_host[2]) {
  LPGP_CHECK(ctx && mat && ginv && dG && r_host && out_host && max_wgs >= 0, "lpgp_test_evidence_grad: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_TEST_FACTORED(ctx, mat, "lpgp_test_evidence_grad");
  LPGP_TRY(evidence_grad_layout(mat, ginv, "lpgp_test_evidence_grad", "the inverse"));
  LPGP_TRY(evidence_grad_layout(mat, dG, "lpgp_test_evidence_grad", "the derivative"));
  return mat_evidence_grad(ctx, mat, ginv, dG, r_host, out_host, max_wgs);
}

int lpgp_test_evidence_grad_diag(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, int32_t bi, const double* v_host, double scalar,
                                 const double* r_host, int32_t max_wgs, double out_host[2]) {
  LPGP_CHECK(ctx && mat && ginv && r_host && out_host && max_wgs >= 0, "lpgp_test_evidence_grad_diag: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_TEST_FACTORED(ctx, mat, "lpgp_test_evidence_grad_diag");
  LPGP_CHECK(bi >= 0 && bi < (int32_t)mat->blocks.size(), "lpgp_test_evidence_grad_diag: bad block %d", bi);
  LPGP_TRY(evidence_grad_layout(mat, ginv, "lpgp_test_evidence_grad_diag", "the inverse"));
  return mat_evidence_grad_diag(ctx, mat, ginv, bi, v_host, scalar, r_host, out_host, max_wgs);
}

}  // extern "C"
