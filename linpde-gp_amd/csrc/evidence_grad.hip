// evidence_grad.hip -- what the gradient of the log marginal likelihood with respect to a hyperparameter theta needs from the
// resident Cholesky factor (Rasmussen & Williams, "Gaussian Processes for Machine Learning", eq. 5.9):
//
//   d/d theta log p(y) = 1/2 w^T (dG/d theta) w - 1/2 tr(G^{-1} dG/d theta),      w = G^{-1} r
//
//   lpgp_mat_inverse             G^{-1} = W^T W,  W = L^{-1}, dense, lower triangle, in a device matrix of its own
//   lpgp_mat_evidence_grad       ( w^T dG w,  tr(G^{-1} dG) )  for an assembled, unfactored dG of the same block layout
//   lpgp_mat_evidence_grad_diag  the same pair for dG = diag(v) + scalar I on one block (a noise variance)
//
// The inverse: W is built column panel by column panel like the inverse diagonal of evidence.hip -- the identity, solved by the
// blocked forward substitution against the TRAILING sub-factor L[j0:, j0:], whose rows above j0 stay the zeros they were cleared
// to -- and W^T W is the fp64 MFMA product in bands of four tile columns from the diagonal down, each over the rows from its first
// column on only (W is lower triangular: (W^T W)_ij = sum_{k >= max(i, j)} W_ki W_kj).  n^3 / 3 + n^3 / 3 flop.
//
// The contraction is the hot path: once per hyperparameter, bound by reading the two lower triangles once (8 n^2 bytes).  A wave
// owns a column (columns are dealt to the waves cyclically, so every wave gets long and short ones), its lanes stream the column
// from the diagonal down, two rows per 16-byte load, off-diagonal entries counted twice.  The padding rows and columns carry an
// identity tail in both matrices (1 * 1 on the diagonal): they are masked by the logical row map.  Every sum is taken in a fixed
// order -- per lane in column order, lanes by shuffles, waves and workgroups by a fixed tree in a second small kernel -- so a call
// returns the same bits every time (no atomics; as evidence_partial_kernel / evidence_final_kernel).
#include <algorithm>
#include <cstring>

#include "lpgp_internal.h"

namespace lpgp {

constexpr int EG_THREADS = 256;
constexpr int EG_WAVES = EG_THREADS / 64;
constexpr int EG_MAX_WGS = 2048;                // partial sums per quantity (eight workgroups per CU keep the loads in flight)
// in-band status of a result: a quiet NaN whose payload no arithmetic produces (the values of evidence.hip)
constexpr unsigned long long EG_NAN_HANDOVER = 0x7FF8000000000001ull;

// sum over the workgroup, valid in thread 0: lanes by shuffles, the four waves as (0 + 1) + (2 + 3); red: 4 doubles of LDS
__device__ __forceinline__ double eg_block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// stage 1: part[b] = sum over the columns of workgroup b of  w_j sum_i f_ij w_i dG_ij,  part[EG_MAX_WGS + b] = sum f_ij Ginv_ij dG_ij
// with f_ij = 1 on the diagonal, 2 below it, 0 where row or column is padding (lrow < 0).  ginv / dg: pn x pn column-major lower
// triangles, leading dimensions lda / ldb (multiples of 128, so every column starts on a 16-byte boundary); pn is even.
__global__ __launch_bounds__(EG_THREADS) void evidence_grad_partial_kernel(const double* __restrict__ ginv, int64_t lda, const double* __restrict__ dg, int64_t ldb,
                                                                           const double* __restrict__ w, const int32_t* __restrict__ lrow, int64_t pn,
                                                                           double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * EG_WAVES + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * EG_WAVES;
  double q = 0.0, t = 0.0;
  for (int64_t j = wave; j < pn; j += nwaves) {
    if (lrow[j] < 0) continue;                   // (uniform over the wave)
    const double* ca = ginv + j * lda;
    const double* cb = dg + j * ldb;
    double cq = 0.0, ct = 0.0;
#pragma unroll 4
    for (int64_t i = (j & ~(int64_t)1) + 2 * lane; i < pn; i += 128) {
      const double2 a = *reinterpret_cast<const double2*>(ca + i);
      const double2 b = *reinterpret_cast<const double2*>(cb + i);
      const double2 wi = *reinterpret_cast<const double2*>(w + i);
      const int2 li = *reinterpret_cast<const int2*>(lrow + i);
      const double f0 = li.x < 0 ? 0.0 : (i > j ? 2.0 : (i == j ? 1.0 : 0.0));
      const double f1 = li.y < 0 ? 0.0 : (i + 1 > j ? 2.0 : 1.0);       // (i + 1 >= j always: i >= j - 1)
      // a masked entry may hold anything, also a NaN: it is selected away, not multiplied by zero
      if (f0 != 0.0) { cq = fma(f0 * wi.x, b.x, cq); ct = fma(f0 * a.x, b.x, ct); }
      if (f1 != 0.0) { cq = fma(f1 * wi.y, b.y, cq); ct = fma(f1 * a.y, b.y, ct); }
    }
    q = fma(w[j], cq, q);
    t += ct;
  }
  q = eg_block_sum(q, red);
  t = eg_block_sum(t, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = q;
    part[EG_MAX_WGS + blockIdx.x] = t;
  }
}

// the same pair for dG = diag(v): part[b] = sum v_i w_i^2, part[EG_MAX_WGS + b] = sum v_i Ginv_ii over the rows of workgroup b;
// v is zero outside the block it belongs to, padding rows are masked
__global__ __launch_bounds__(EG_THREADS) void evidence_grad_diag_partial_kernel(const double* __restrict__ ginv, int64_t lda, const double* __restrict__ v,
                                                                                const double* __restrict__ w, const int32_t* __restrict__ lrow, int64_t pn,
                                                                                double* __restrict__ part) {
  __shared__ double red[4];
  double q = 0.0, t = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)EG_THREADS + threadIdx.x; i < pn; i += (int64_t)gridDim.x * EG_THREADS) {
    if (lrow[i] < 0) continue;
    const double vi = v[i], wi = w[i];
    q = fma(vi * wi, wi, q);
    t = fma(vi, ginv[i * (lda + 1)], t);
  }
  q = eg_block_sum(q, red);
  t = eg_block_sum(t, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = q;
    part[EG_MAX_WGS + blockIdx.x] = t;
  }
}

// stage 2: one workgroup adds the nwg <= EG_MAX_WGS partials of each quantity, thread t those of the workgroups t, t + 256, ...
__global__ __launch_bounds__(EG_THREADS) void evidence_grad_final_kernel(const double* __restrict__ part, int nwg, const int* __restrict__ info,
                                                                         double* __restrict__ out) {
  __shared__ double red[4];
  double q = 0.0, t = 0.0;
  for (int b = threadIdx.x; b < nwg; b += EG_THREADS) {
    q += part[b];
    t += part[EG_MAX_WGS + b];
  }
  q = eg_block_sum(q, red);
  t = eg_block_sum(t, red);
  if (threadIdx.x == 0) {
    out[0] = *info < 0 ? __longlong_as_double((long long)EG_NAN_HANDOVER) : q;
    out[1] = t;
  }
}

// ones on the diagonal of the cleared pn x pn matrix
__global__ __launch_bounds__(EG_THREADS) void unit_diag_kernel(double* __restrict__ a, int64_t ld, int64_t pn) {
  const int64_t i = blockIdx.x * (int64_t)EG_THREADS + threadIdx.x;
  if (i < pn) a[i * (ld + 1)] = 1.0;
}

// lpgp_mat_inverse: out->a (lower triangle; leading dimension out->lr_cap >= pn) <- G^{-1} = W^T W from the factor in mat
int mat_inverse_into(lpgp_ctx* ctx, lpgp_mat* mat, lpgp_mat* out) {
  const int64_t pn = mat->pn, panel = std::min<int64_t>(ctx->inverse_diag_panel, pn);
  const int T = (int)(pn / TILE), BW = 4;
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  DevBuf wbuf;                                   // W = L^{-1}, pn x pn (reuse is ordered on the panel stream, which the blocked solve joins at its end)
  LPGP_TRY(DevBuf::pool(ctx, (size_t)pn * pn * sizeof(double), &wbuf));
  double* const W = wbuf.as();
  LPGP_HIP(hipMemsetAsync(W, 0, (size_t)pn * pn * sizeof(double), st));
  hipLaunchKernelGGL(unit_diag_kernel, dim3((unsigned)((pn + EG_THREADS - 1) / EG_THREADS)), dim3(EG_THREADS), 0, st, W, pn, pn);
  LPGP_HIP(hipGetLastError());
  for (int64_t j0 = 0; j0 < pn; j0 += panel) {
    const int64_t rows = pn - j0, pc = std::min(panel, rows);
    // against the trailing sub-factor L[j0:, j0:] (as inverse_diag_device)
    LPGP_TRY(trsm_lower_blocked(ctx, F.trailing((int)(j0 / TILE)), rows / TILE, W + j0 * (pn + 1), pn, pc));
  }
  // out[c0:, c0 : c0 + BW] = W[c0:, c0:]^T W[c0:, c0 : c0 + BW], band by band (the form of lpgp_mat_sub_inner); the tiles above the
  // diagonal inside a band are written and never read
  for (int c0 = 0; c0 < T; c0 += BW) {
    GemmArgs g;
    g.A = W + (int64_t)c0 * TILE * (pn + 1); g.B = g.A; g.C = out->a + (int64_t)c0 * TILE * (out->lr_cap + 1);
    g.lda = pn; g.ldb = pn; g.ldc = out->lr_cap;
    g.mt = T - c0; g.nt = std::min(BW, T - c0); g.k = (int)(pn - (int64_t)c0 * TILE); g.alpha = 1.0; g.beta = 0.0;
    g.tri = 0;
    LPGP_TRY(launch_gemm(ctx, st, 1, 1, g, LPGP_K_GEMM));
  }
  return 0;        // asynchronous: consumers are ordered behind it on the main stream
}

// workgroups of a stage-1 launch with `per` columns or rows each; max_wgs > 0 (the test hooks') caps them below what the size asks for
static int eg_wgs(int64_t pn, int per, int max_wgs) {
  const int nwg = (int)std::min<int64_t>((pn + per - 1) / per, EG_MAX_WGS);
  return max_wgs > 0 ? std::min(nwg, max_wgs) : nwg;
}

static int eg_finish(lpgp_ctx* ctx, hipStream_t st, double* d_part, int nwg, double* d_out, double out_host[2], StreamDrain* drain, const char* fn) {
  hipLaunchKernelGGL(evidence_grad_final_kernel, dim3(1), dim3(EG_THREADS), 0, st, (const double*)d_part, nwg, (const int*)ctx->d_info, d_out);
  LPGP_HIP(hipGetLastError());
  LPGP_HIP(hipMemcpyAsync(out_host, d_out, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  ctx->evidence_d2h_bytes += (int64_t)(2 * sizeof(double));
  LPGP_TRY(drain->wait());
  unsigned long long u;
  std::memcpy(&u, &out_host[0], sizeof u);
  LPGP_CHECK(u != EG_NAN_HANDOVER, "%s: resident single-vector solve: a hand-over between workgroups timed out; set LPGP_TRSV_RESIDENT=0", fn);
  return 0;
}

// `other` (the dense inverse, an assembled derivative) lies over the blocks `mat` views: same context, same block layout, not factored
int evidence_grad_layout(const lpgp_mat* mat, const lpgp_mat* other, const char* fn, const char* what) {
  LPGP_CHECK(other->ctx == mat->ctx && !other->poisoned, "%s: %s belongs to another context or is undefined", fn, what);
  LPGP_CHECK(other->pn == mat->pn && other->blocks.size() == mat->blocks.size() && other->hidden.empty(),
             "%s: %s has another block layout than the matrix (%lld padded rows in %d blocks against %lld in %d)", fn, what, (long long)other->pn,
             (int)other->blocks.size(), (long long)mat->pn, (int)mat->blocks.size());
  for (size_t b = 0; b < mat->blocks.size(); ++b)
    LPGP_CHECK(other->blocks[b].n == mat->blocks[b].n && other->blocks[b].poff == mat->blocks[b].poff,
               "%s: block %d of %s has %lld rows, the matrix has %lld", fn, (int)b, what, (long long)other->blocks[b].n, (long long)mat->blocks[b].n);
  LPGP_CHECK(other->pn_fact == 0, "%s: %s must not be factored", fn, what);
  return 0;
}

// lpgp_mat_evidence_grad: w = G^{-1} r through the single-vector path (trsv.hip), the streaming contraction, ONE read-back of 16 bytes
int mat_evidence_grad(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, const lpgp_mat* dG, const double* r_host, double out_host[2],
                      int max_wgs) {
  const int64_t pn = mat->pn, T = pn / TILE;
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  std::vector<double> h;
  ev_stage(mat, &r_host, 1, &h);                 // (the host staging of evidence.hip)
  // [w (r on entry) | lrow] as staged, the scratch of the solve (+ 2 ticket words), the partials, the result
  const size_t o_tmp = h.size(), o_part = o_tmp + (size_t)pn + 2, o_out = o_part + 2 * EG_MAX_WGS;
  DevBuf buf;
  LPGP_TRY(DevBuf::pool(ctx, (o_out + 2) * sizeof(double), &buf));
  double* const d = buf.as();
  StreamDrain drain{st};                         // (the staging vector and the caller's array are borrowed by the copies)
  LPGP_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st));
  ctx->evidence_h2d_bytes += (int64_t)(h.size() * sizeof(double));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  LPGP_TRY(solve_vec(ctx, F, T, d, d + o_tmp, ctx->d_info));
  const int nwg = eg_wgs(pn, EG_WAVES, max_wgs);
  hipLaunchKernelGGL(evidence_grad_partial_kernel, dim3((unsigned)nwg), dim3(EG_THREADS), 0, st, (const double*)ginv->a, ginv->lr_cap, (const double*)dG->a,
                     dG->lr_cap, (const double*)d, reinterpret_cast<const int32_t*>(d + pn), pn, d + o_part);
  LPGP_HIP(hipGetLastError());
  return eg_finish(ctx, st, d + o_part, nwg, d + o_out, out_host, &drain, "lpgp_mat_evidence_grad");
}

// lpgp_mat_evidence_grad_diag: the pair for dG = diag(v) + scalar I on block bi, from w and the diagonal of the inverse
int mat_evidence_grad_diag(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, int32_t bi, const double* v_host, double scalar, const double* r_host,
                           double out_host[2], int max_wgs) {
  const int64_t pn = mat->pn, T = pn / TILE;
  const lpgp_block& B = mat->blocks[(size_t)bi];
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  std::vector<double> h, v((size_t)mat->n, 0.0);     // the diagonal of dG over all logical rows: zero outside block bi
  for (int64_t i = 0; i < B.n; ++i) v[(size_t)(B.off + i)] = v_host ? scalar + v_host[i] : scalar;
  const double* vecs[2] = {r_host, v.data()};
  ev_stage(mat, vecs, 2, &h);
  // [w (r on entry) | v | lrow] as staged, the scratch of the solve (+ 2 ticket words), the partials, the result
  const size_t o_tmp = h.size(), o_part = o_tmp + (size_t)pn + 2, o_out = o_part + 2 * EG_MAX_WGS;
  DevBuf buf;
  LPGP_TRY(DevBuf::pool(ctx, (o_out + 2) * sizeof(double), &buf));
  double* const d = buf.as();
  StreamDrain drain{st};
  LPGP_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st));
  ctx->evidence_h2d_bytes += (int64_t)(h.size() * sizeof(double));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  LPGP_TRY(solve_vec(ctx, F, T, d, d + o_tmp, ctx->d_info));
  const int nwg = eg_wgs(pn, EG_THREADS, max_wgs);
  hipLaunchKernelGGL(evidence_grad_diag_partial_kernel, dim3((unsigned)nwg), dim3(EG_THREADS), 0, st, (const double*)ginv->a, ginv->lr_cap,
                     (const double*)(d + pn), (const double*)d, reinterpret_cast<const int32_t*>(d + 2 * pn), pn, d + o_part);
  LPGP_HIP(hipGetLastError());
  return eg_finish(ctx, st, d + o_part, nwg, d + o_out, out_host, &drain, "lpgp_mat_evidence_grad_diag");
}

}  // namespace lpgp
