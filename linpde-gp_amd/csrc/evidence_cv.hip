// evidence_cv.hip -- leave-fold-out cross-validation from the resident factor: the predictive distribution of a whole fold B of
// observations given all the others (Rasmussen & Williams, "Gaussian Processes for Machine Learning", section 5.4.2: the block form
// of eqs. 5.10 - 5.12).  With P = G^{-1} (lpgp_mat_inverse) and w = G^{-1} r:
//
//   S = P[B, B] = C C^T          (b x b, b = |B|)
//   mean_B  = y_B - S^{-1} w_B = y_B - C^{-T} t,   t = C^{-1} w_B
//   Sigma_B = S^{-1} = C^{-T} C^{-1}               (covariance of the noisy y_B; var = its diagonal, var_i = sum_{k >= i} (C^{-1})_ki^2)
//   log p(y_B | y_-B) = -1/2 || t ||^2 + sum_i log C_ii - b/2 log 2 pi
//
// b = 1 is lpgp_mat_loo, B = all rows the log marginal likelihood.  No fold needs a conditioning of its own.
//
// Tile path, b <= 128, many folds per launch: cv_gather_kernel writes each fold's S into a 128 x 128 scratch tile (identity tail
// behind row b, as the project pads everywhere), cv_factor_kernel runs the tile Cholesky of the factorisation (potrf_tile.h: C and
// C^{-1} explicitly) with one workgroup per fold, cv_epilogue_kernel forms the formulas above with one workgroup per fold.  Three
// launches: the tile Cholesky loads its tile by LDS-DMA, which a gather inside the same workgroup would have to be made visible to.
// 256 KiB of scratch per fold, so the folds run in batches (option "cv_fold_batch", default 512 = 128 MiB).
// Large path, b > 128, one fold at a time through the drivers of the library: S gathered into a scratch matrix of one block,
// factored (lpgp_potrf), quad and log det S from mat_evidence, S^{-1} w_B from the single-vector solve, the variances from
// inverse_diag_device, Sigma_B (on request) from lpgp_mat_inverse.
//
// Every sum has a fixed order -- a thread in index order, a workgroup by the tree of evidence.hip, the total over the folds by one
// thread in fold order -- and nothing is accumulated by atomics: a call returns the same bits every time.  O(n) numbers cross the bus,
// and the covariances if they are asked for.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lpgp_internal.h"
#include "kernel_util.h"
#include "potrf_tile.h"
#include "fold_table.h"

namespace lpgp {

constexpr int CV_THREADS = 256;
constexpr int64_t CV_FOLD_DOUBLES = 2 * (int64_t)TILE * TILE;      // scratch of a tile fold: [S, then C | C^{-1}]
constexpr double CV_HALF_LOG_2PI = 0.91893853320467274178;
constexpr unsigned long long CV_NAN_HANDOVER = 0x7FF8000000000001ull;     // (the value of evidence.hip)

// the fold table on the device (fold_table.h): members of fold f are prow[start[f] .. start[f + 1]); workgroup k of a tile launch
// works on fold ids[k]
struct CvFolds {
  const int32_t* prow;
  const int32_t* start;
  const int32_t* ids;
};

// sum over the workgroup: lanes by shuffles, the four waves as (0 + 1) + (2 + 3); red: 4 doubles of LDS (ev_block_sum of evidence.hip)
__device__ __forceinline__ double cv_block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// scratch tile of fold ids[blockIdx.x] <- [P[B, B], 0; 0, I], all 128 x 128 entries (column-major, leading dimension 128); P is read from its
// lower triangle.  blockIdx.y: eight columns of the tile.
__global__ __launch_bounds__(CV_THREADS) void cv_gather_kernel(const double* __restrict__ P, int64_t ldp, CvFolds F, double* __restrict__ tiles) {
  const int f = F.ids[blockIdx.x], s = F.start[f], b = F.start[f + 1] - s;
  double* a = tiles + (int64_t)blockIdx.x * CV_FOLD_DOUBLES;
  const int i = threadIdx.x & (TILE - 1);
  const int64_t pi = i < b ? F.prow[s + i] : -1;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = blockIdx.y * 8 + (threadIdx.x >> 7) * 4 + c;
    double v = i == j ? 1.0 : 0.0;
    if (i < b && j < b) {
      const int64_t pj = F.prow[s + j];
      v = P[(pi > pj ? pi : pj) + (pi > pj ? pj : pi) * ldp];
    }
    a[i + j * TILE] = v;
  }
}

// one workgroup per fold: S <- C (lower, zeros above the diagonal), C^{-1} behind it; status[blockIdx.x]: first pivot that is not positive, from 1
__global__ __launch_bounds__(TILE_WAVES * 64) void cv_factor_kernel(double* __restrict__ tiles, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* a = tiles + (int64_t)blockIdx.x * CV_FOLD_DOUBLES;
  potrf_tile_body<true>(a, TILE, a + TILE * TILE, status + blockIdx.x, 0, sm);      // (true: the Newton sign for C^{-1}, potrf_tile.h)
}

// one workgroup per fold: the formulas at the top from C and X = C^{-1}.  mean / var: per member (the order of prow); logp: per fold;
// cov: NULL, or fold ids[k]'s b x b covariance goes to cov + cov_off[k] (C order).  The rows behind b are the identity's and w_B
// is zero there: every loop stops at b.
__global__ __launch_bounds__(CV_THREADS) void cv_epilogue_kernel(const double* __restrict__ tiles, const double* __restrict__ w, const double* __restrict__ y,
                                                                 CvFolds F, double* __restrict__ mean, double* __restrict__ var, double* __restrict__ logp,
                                                                 double* __restrict__ cov, const int64_t* __restrict__ cov_off) {
  __shared__ double wB[TILE], t[TILE], red[4];
  const int f = F.ids[blockIdx.x], s = F.start[f], b = F.start[f + 1] - s, tid = threadIdx.x;
  const double* C = tiles + (int64_t)blockIdx.x * CV_FOLD_DOUBLES;
  const double* X = C + TILE * TILE;
  if (tid < TILE) wB[tid] = tid < b ? w[F.prow[s + tid]] : 0.0;
  __syncthreads();
  double tk = 0.0, lg = 0.0;
  if (tid < b) {                                 // t = C^{-1} w_B: row tid, columns in order
    for (int j = 0; j <= tid; ++j) tk = fma(X[tid + j * TILE], wB[j], tk);
    lg = log(C[tid * (TILE + 1)]);
  }
  if (tid < TILE) t[tid] = tk;
  const double quad = cv_block_sum(tk * tk, red);
  const double lsum = cv_block_sum(lg, red);     // (its barriers also publish t)
  if (tid < b) {                                 // C^{-T} t and the diagonal of C^{-T} C^{-1}: column tid of X from the diagonal down
    double u = 0.0, v = 0.0;
    for (int k = tid; k < b; ++k) {
      const double x = X[k + tid * TILE];
      u = fma(x, t[k], u);
      v = fma(x, x, v);
    }
    mean[s + tid] = y[F.prow[s + tid]] - u;
    var[s + tid] = v;
  }
  if (tid == 0) logp[f] = lsum - 0.5 * quad - (double)b * CV_HALF_LOG_2PI;
  if (cov != nullptr) {
    double* out = cov + cov_off[blockIdx.x];
    for (int e = tid; e < b * b; e += CV_THREADS) {
      const int i = e / b, j = e - i * b;
      double acc = 0.0;
      for (int k = i > j ? i : j; k < b; ++k) acc = fma(X[k + i * TILE], X[k + j * TILE], acc);
      out[e] = acc;
    }
  }
}

// logp[nfolds] = logp[0] + logp[1] + ... in fold order, by one thread (the others fetch); a timed-out hand-over of the solve of w: its NaN
__global__ __launch_bounds__(CV_THREADS) void cv_total_kernel(double* __restrict__ logp, int nfolds, const int* __restrict__ info) {
  __shared__ double buf[CV_THREADS];
  double sum = 0.0;
  for (int f0 = 0; f0 < nfolds; f0 += CV_THREADS) {
    const int cnt = nfolds - f0 < CV_THREADS ? nfolds - f0 : CV_THREADS;
    if ((int)threadIdx.x < cnt) buf[threadIdx.x] = logp[f0 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < cnt; ++i) sum += buf[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) logp[nfolds] = *info < 0 ? __longlong_as_double((long long)CV_NAN_HANDOVER) : sum;
}

// large path: the scratch matrix (one block: padded row == row) <- P[B, B], its lower triangle and all of its diagonal tiles
__global__ __launch_bounds__(CV_THREADS) void cv_gather_large_kernel(const double* __restrict__ P, int64_t ldp, const int32_t* __restrict__ prow, int b,
                                                                     double* __restrict__ a, int64_t lda) {
  const int i = blockIdx.x * CV_THREADS + threadIdx.x, j = blockIdx.y + blockIdx.z * 65535;
  if (i >= b || j >= b || (i < j && i / TILE != j / TILE)) return;
  const int64_t pi = prow[i], pj = prow[j];
  a[i + (int64_t)j * lda] = P[(pi > pj ? pi : pj) + (pi > pj ? pj : pi) * ldp];
}

// large path: mean = y_B - S^{-1} w_B and var = diag(S^{-1}) into the members' slots
__global__ __launch_bounds__(CV_THREADS) void cv_large_epilogue_kernel(const double* __restrict__ x, const double* __restrict__ dg, const double* __restrict__ y,
                                                                       const int32_t* __restrict__ prow, int b, double* __restrict__ mean, double* __restrict__ var) {
  const int i = blockIdx.x * CV_THREADS + threadIdx.x;
  if (i >= b) return;
  mean[i] = y[prow[i]] - x[i];
  var[i] = dg[i];
}

namespace {

struct LPGP_LOCAL MatGuard {                     // a scratch matrix of the large path
  lpgp_mat* m = nullptr;
  ~MatGuard() { if (m) (void)lpgp_mat_destroy(m); }
};

// what the call keeps on the device: [w (r on entry) | y | lrow] as staged, the scratch of the solve, [mean | var] per member and
// [logp | total]; the table as int32: [prow | start | tile ids | status per tile fold | status of the solve of w]
struct CvDevice {
  double *w, *y, *mean, *var, *logp;
  int32_t *prow, *start, *ids;
  int *status, *solve_info;
};

int cv_upload_bytes(lpgp_ctx* ctx, void* dst, const void* src, size_t bytes) {
  LPGP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->s_main));
  ctx->evidence_h2d_bytes += (int64_t)bytes;
  return 0;
}

// one fold of more than 128 rows; w_pad: w in the padded layout, on the host; *logp_out and cov_out (NULL: not asked) are the host's
int cv_large_fold(lpgp_ctx* ctx, const lpgp_mat* ginv, const FoldTable& tab, int32_t f, const CvDevice& D, const double* w_pad, double* logp_out,
                  double* cov_out) {
  const int64_t s = tab.start[(size_t)f], b = tab.size(f), spn = round_up(b, TILE);
  hipStream_t st = ctx->s_main;
  MatGuard S;
  LPGP_TRY(lpgp_mat_create(ctx, spn, &S.m));
  LPGP_CHECK(lpgp_mat_add_block(ctx, S.m, b) == 0, "lpgp_mat_cv: fold %d: %s", f, last_error());
  const unsigned gy = (unsigned)(b < 65535 ? b : 65535), gz = (unsigned)((b + 65534) / 65535);
  hipLaunchKernelGGL(cv_gather_large_kernel, dim3((unsigned)((b + CV_THREADS - 1) / CV_THREADS), gy, gz), dim3(CV_THREADS), 0, st, (const double*)ginv->a,
                     ginv->lr_cap, (const int32_t*)(D.prow + s), (int)b, S.m->a, S.m->lr_cap);
  LPGP_HIP(hipGetLastError());
  // S is factored with the Newton sign in the tile Cholesky (TileForm::newton): mean, variances and covariance of the fold are read off
  // S^{-1}, where a backward error of the factor is multiplied by cond(S) -- with the factorisation's own sign the 150-row fold of
  // tests/test_gpu_cv.py (cond_2(S) = 5e3) was 17 x LAPACK's distance from the truth.  The resident panel chain carries the
  // factorisation's sign, so a factorisation of this form runs without it: per-tile launches, the schedule of LPGP_CHAIN_RESIDENT=-1.
  int32_t info = 0;
  LPGP_TRY(potrf_mat(ctx, S.m, &info, TileForm::newton));
  LPGP_CHECK(info == 0, "lpgp_mat_cv: fold %d: pivot %d of G^-1[B, B] is not positive", f, info);
  std::vector<double> wB((size_t)spn, 0.0);      // (single block: the padded layout is the logical one with a zero tail)
  for (int64_t i = 0; i < b; ++i) wB[(size_t)i] = w_pad[tab.prow[(size_t)(s + i)]];
  double ev[2];
  LPGP_TRY(mat_evidence(ctx, S.m, wB.data(), ev));
  *logp_out = 0.5 * ev[1] - 0.5 * ev[0] - (double)b * CV_HALF_LOG_2PI;
  FactorView F;
  LPGP_TRY(factor_view(S.m, &F));
  // x (w_B on entry), the scratch of the solve (+ 2 ticket words), diag(S^{-1})
  DevBuf buf;
  LPGP_TRY(DevBuf::pool(ctx, (size_t)(3 * spn + 2) * sizeof(double), &buf));
  double* const x = buf.as();
  double* const dg = x + 2 * spn + 2;
  MatGuard inv;
  int solve_info = 0;
  StreamDrain drain{st};
  LPGP_TRY(ev_upload(ctx, x, wB));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  LPGP_TRY(solve_vec(ctx, F, spn / TILE, x, x + spn, ctx->d_info));
  LPGP_HIP(hipMemcpyAsync(&solve_info, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, st));
  ctx->evidence_d2h_bytes += (int64_t)sizeof(int);
  LPGP_TRY(inverse_diag_device(ctx, S.m, dg));
  hipLaunchKernelGGL(cv_large_epilogue_kernel, dim3((unsigned)((b + CV_THREADS - 1) / CV_THREADS)), dim3(CV_THREADS), 0, st, (const double*)x, (const double*)dg,
                     (const double*)D.y, (const int32_t*)(D.prow + s), (int)b, D.mean + s, D.var + s);
  LPGP_HIP(hipGetLastError());
  if (cov_out) {
    LPGP_TRY(lpgp_mat_inverse(ctx, S.m, &inv.m));
    // column j of the lower triangle lands in row j of the C-order result: its upper triangle; mirrored below
    LPGP_HIP(hipMemcpy2DAsync(cov_out, (size_t)b * sizeof(double), inv.m->a, (size_t)inv.m->lr_cap * sizeof(double), (size_t)b * sizeof(double), (size_t)b,
                              hipMemcpyDeviceToHost, st));
    ctx->evidence_d2h_bytes += b * b * (int64_t)sizeof(double);
  }
  LPGP_TRY(drain.wait());
  LPGP_CHECK(solve_info >= 0, "lpgp_mat_cv: resident single-vector solve: a hand-over between workgroups timed out; set LPGP_TRSV_RESIDENT=0");
  if (cov_out)
    for (int64_t i = 1; i < b; ++i)
      for (int64_t j = 0; j < i; ++j) cov_out[i * b + j] = cov_out[j * b + i];
  return 0;
}

}  // namespace

int mat_cv(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, const double* r_host, const double* y_host, const int32_t* fold_of, int32_t nfolds,
           double* mean_host, double* var_host, double* logp_host, double* cov_host) {
  const int64_t pn = mat->pn, n = mat->n, T = pn / TILE;
  hipStream_t st = ctx->s_main;
  FoldTable tab;
  std::string err;
  LPGP_CHECK(fold_table_build(mat->blocks.data(), (int)mat->blocks.size(), fold_of, n, nfolds, &tab, &err) == 0, "lpgp_mat_cv: %s", err.c_str());
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  const int64_t m = tab.members(), ntile = (int64_t)tab.tile.size(), batch = std::min<int64_t>(ctx->cv_fold_batch, ntile);
  std::vector<double> h, res((size_t)(2 * m + nfolds + 1)), w_pad, tile_cov, cov;
  const double* vecs[2] = {r_host, y_host};
  ev_stage(mat, vecs, 2, &h);
  std::vector<int32_t> it(tab.prow);
  it.insert(it.end(), tab.start.begin(), tab.start.end());
  it.insert(it.end(), tab.tile.begin(), tab.tile.end());
  const size_t o_status = it.size();
  it.resize(o_status + (size_t)ntile + 1, 0);    // the status words start at zero
  std::vector<int32_t> status((size_t)ntile + 1);
  std::vector<double> large_logp(tab.large.size());
  if (cov_host) cov.resize((size_t)tab.cov_off.back());

  const size_t o_tmp = h.size(), o_res = o_tmp + (size_t)pn + 2;
  DevBuf dbuf, ibuf, tbuf, cbuf, obuf;
  LPGP_TRY(DevBuf::pool(ctx, (o_res + res.size()) * sizeof(double), &dbuf));
  LPGP_TRY(DevBuf::pool(ctx, it.size() * sizeof(int32_t), &ibuf));
  if (ntile > 0) LPGP_TRY(DevBuf::pool(ctx, (size_t)(batch * CV_FOLD_DOUBLES) * sizeof(double), &tbuf));
  const bool tile_cov_wanted = cov_host && ntile > 0;
  if (tile_cov_wanted) {
    tile_cov.resize((size_t)tab.tile_cov_off.back());
    LPGP_TRY(DevBuf::pool(ctx, tile_cov.size() * sizeof(double), &cbuf));
    LPGP_TRY(DevBuf::pool(ctx, tab.tile_cov_off.size() * sizeof(int64_t), &obuf));
  }
  double* const d = dbuf.as();
  int32_t* const di = ibuf.as<int32_t>();
  CvDevice D;
  D.w = d; D.y = d + pn; D.mean = d + o_res; D.var = D.mean + m; D.logp = D.var + m;
  D.prow = di; D.start = di + m; D.ids = D.start + nfolds + 1;
  D.status = reinterpret_cast<int*>(di + o_status); D.solve_info = D.status + ntile;

  StreamDrain drain{st};                         // (the staging vectors are borrowed by the copies)
  LPGP_TRY(ev_upload(ctx, d, h));
  LPGP_TRY(cv_upload_bytes(ctx, di, it.data(), it.size() * sizeof(int32_t)));
  if (tile_cov_wanted) LPGP_TRY(cv_upload_bytes(ctx, obuf.as<void>(), tab.tile_cov_off.data(), tab.tile_cov_off.size() * sizeof(int64_t)));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  LPGP_TRY(solve_vec(ctx, F, T, d, d + o_tmp, ctx->d_info));
  LPGP_HIP(hipMemcpyAsync(D.solve_info, ctx->d_info, sizeof(int), hipMemcpyDeviceToDevice, st));     // (the large path uses the context's word again)

  if (ntile > 0) {
    const size_t shmem = (size_t)TILE_LDS_DOUBLES * sizeof(double);
    LPGP_TRY(ensure_lds_attr(ctx, reinterpret_cast<const void*>(&cv_factor_kernel), shmem));
    for (int64_t k = 0; k < fold_num_batches(ntile, batch); ++k) {
      int64_t k0, cnt;
      fold_batch(ntile, batch, k, &k0, &cnt);
      const CvFolds Fk{D.prow, D.start, D.ids + k0};
      hipLaunchKernelGGL(cv_gather_kernel, dim3((unsigned)cnt, TILE / 8), dim3(CV_THREADS), 0, st, (const double*)ginv->a, ginv->lr_cap, Fk, tbuf.as());
      hipLaunchKernelGGL(cv_factor_kernel, dim3((unsigned)cnt), dim3(TILE_WAVES * 64), shmem, st, tbuf.as(), D.status + k0);
      hipLaunchKernelGGL(cv_epilogue_kernel, dim3((unsigned)cnt), dim3(CV_THREADS), 0, st, (const double*)tbuf.as(), (const double*)D.w, (const double*)D.y, Fk,
                         D.mean, D.var, D.logp, tile_cov_wanted ? cbuf.as() : (double*)nullptr,
                         tile_cov_wanted ? (const int64_t*)(obuf.as<int64_t>() + k0) : (const int64_t*)nullptr);
      LPGP_HIP(hipGetLastError());
    }
  }
  if (!tab.large.empty()) {
    w_pad.resize((size_t)pn);
    LPGP_TRY(ev_download(ctx, w_pad.data(), D.w, (size_t)pn));
    LPGP_HIP(hipStreamSynchronize(st));
    for (size_t q = 0; q < tab.large.size(); ++q) {
      const int32_t f = tab.large[q];
      LPGP_TRY(cv_large_fold(ctx, ginv, tab, f, D, w_pad.data(), &large_logp[q], cov_host ? cov.data() + tab.cov_off[(size_t)f] : nullptr));
      LPGP_TRY(cv_upload_bytes(ctx, D.logp + f, &large_logp[q], sizeof(double)));
    }
  }
  hipLaunchKernelGGL(cv_total_kernel, dim3(1), dim3(CV_THREADS), 0, st, D.logp, (int)nfolds, (const int*)D.solve_info);
  LPGP_HIP(hipGetLastError());
  LPGP_TRY(ev_download(ctx, res.data(), D.mean, res.size()));
  LPGP_HIP(hipMemcpyAsync(status.data(), D.status, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  ctx->evidence_d2h_bytes += (int64_t)(status.size() * sizeof(int32_t));
  if (tile_cov_wanted) LPGP_TRY(ev_download(ctx, tile_cov.data(), cbuf.as(), tile_cov.size()));
  LPGP_TRY(drain.wait());

  for (int64_t k = 0; k < ntile; ++k)
    LPGP_CHECK(status[(size_t)k] == 0, "lpgp_mat_cv: fold %d: pivot %d of G^-1[B, B] is not positive", tab.tile[(size_t)k], status[(size_t)k]);
  unsigned long long bits;
  std::memcpy(&bits, &res[(size_t)(2 * m + nfolds)], sizeof bits);
  LPGP_CHECK(bits != CV_NAN_HANDOVER, "lpgp_mat_cv: resident single-vector solve: a hand-over between workgroups timed out; set LPGP_TRSV_RESIDENT=0");
  // everything succeeded: only now the caller's arrays are written
  const double nan = std::nan("");
  std::fill(mean_host, mean_host + n, nan);
  std::fill(var_host, var_host + n, nan);
  for (int64_t at = 0; at < m; ++at) {
    mean_host[tab.lrow[(size_t)at]] = res[(size_t)at];
    var_host[tab.lrow[(size_t)at]] = res[(size_t)(m + at)];
  }
  std::memcpy(logp_host, res.data() + 2 * m, (size_t)(nfolds + 1) * sizeof(double));
  if (cov_host) {
    for (int64_t k = 0; k < ntile; ++k) {
      const int32_t f = tab.tile[(size_t)k];
      std::memcpy(cov.data() + tab.cov_off[(size_t)f], tile_cov.data() + tab.tile_cov_off[(size_t)k], (size_t)tab.size(f) * tab.size(f) * sizeof(double));
    }
    std::memcpy(cov_host, cov.data(), cov.size() * sizeof(double));
  }
  return 0;
}

}  // namespace lpgp
