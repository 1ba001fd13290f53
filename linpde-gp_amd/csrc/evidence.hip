// evidence.hip -- what a GP user reads off the resident Cholesky factor first: the two terms of the log marginal likelihood
// and the leave-one-out predictive distribution of every observation (Rasmussen & Williams, "Gaussian Processes for Machine
// Learning", eq. 2.30 / 5.8 and eqs. 5.10 - 5.12; probnum `Normal.logpdf` on `L(prior)(X)` for the reference's users).
//
//   lpgp_mat_evidence      r^T G^{-1} r = || L^{-1} r ||^2   and   log det G = 2 sum_i log L_ii                  (eq. 2.30)
//   lpgp_mat_inverse_diag  diag(G^{-1})_j = sum_{i >= j} (L^{-1})_{ij}^2
//   lpgp_mat_loo           mean_i = y_i - w_i / d_i,  var_i = 1 / d_i,
//                          logp_i = 1/2 log d_i - 1/2 w_i^2 / d_i - 1/2 log 2 pi,   w = G^{-1} r,  d = diag(G^{-1})   (eqs. 5.10 - 5.12)
//
// Nothing of size n^2 reaches the host: the identity right-hand side is written on the device, panel by panel, solved by the
// blocked forward substitution and reduced to one number per column there; the host sees O(n) doubles.
//
// The inverse diagonal solves each column panel against the TRAILING sub-factor only: the rows of L^{-1} e_j above j are exact
// zeros and (L^{-1} e_j)[j0:] = (L[j0:, j0:])^{-1} e_{j - j0}, so panel [j0, j0 + pc) is a forward substitution with the factor
// that starts at tile row j0 / 128 -- the blocked driver as it is, handed the pointers of that tile (at j0 = 0 the call
// lpgp_trsm_lower makes).  Work: sum over the panels of (pn - j0)^2 pc flop -> n^3 / 3 as the panels get narrow against n, the
// cost of the factorisation itself (full-height solves would be n^3).
//
// Every sum is taken in a fixed order -- per thread in row order, the 64 lanes of a wave by shuffles, the waves of a workgroup
// and then the workgroups' partials by a fixed tree -- so a call returns the same bits every time (no atomics; as
// trmm_reduce_kernel and the dots of pcg.hip).  The reductions read n doubles and n diagonal entries: HBM-read bound and small.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lpgp_internal.h"

namespace lpgp {

constexpr int EV_THREADS = 256;
constexpr int EV_MAX_WGS = 256;                 // partial sums per quantity: one workgroup of the final kernel adds them
// in-band status of a result: a quiet NaN whose payload no arithmetic produces
constexpr unsigned long long EV_NAN_HANDOVER = 0x7FF8000000000001ull;     // a hand-over of the resident single-vector solve timed out
constexpr unsigned long long EV_NAN_PADDING = 0x7FF8000000000002ull;      // a padding row of the factor is not the identity's

// sum over the workgroup, valid in thread 0: lanes by shuffles, the four waves as (0 + 1) + (2 + 3); red: 4 doubles of LDS
__device__ __forceinline__ double ev_block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();                               // (red may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// stage 1 of the evidence: workgroup b adds  z_i^2  and  log L_ii  over the padded rows i = b * 256 + t, + gridDim.x * 256, ...
// lrow[i] < 0 marks a padding row: its factor row is the identity's and its residual is zero, so it adds z^2 = 0 and log 1 = 0
// like any other row -- the kernel CHECKS that (part[2 * EV_MAX_WGS + b] counts the rows where it does not hold), it does not mask.
__global__ __launch_bounds__(EV_THREADS) void evidence_partial_kernel(const double* __restrict__ z, const double* __restrict__ L, int64_t ld,
                                                                      const int32_t* __restrict__ lrow, int64_t pn, double* __restrict__ part) {
  __shared__ double red[4];
  double q = 0.0, l = 0.0, bad = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)EV_THREADS + threadIdx.x; i < pn; i += (int64_t)gridDim.x * EV_THREADS) {
    const double zi = z[i], d = L[i * (ld + 1)];
    q = fma(zi, zi, q);
    l += log(d);
    if (lrow[i] < 0 && !(d == 1.0 && zi == 0.0)) bad += 1.0;
  }
  q = ev_block_sum(q, red);
  l = ev_block_sum(l, red);
  bad = ev_block_sum(bad, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = q;
    part[EV_MAX_WGS + blockIdx.x] = l;
    part[2 * EV_MAX_WGS + blockIdx.x] = bad;
  }
}

__device__ __forceinline__ double ev_status_nan(unsigned long long bits) { return __longlong_as_double((long long)bits); }

// stage 2: one workgroup adds the nwg <= 256 partials of each quantity;  out = { || z ||^2, 2 sum log L_ii }
__global__ __launch_bounds__(EV_THREADS) void evidence_final_kernel(const double* __restrict__ part, int nwg, const int* __restrict__ info,
                                                                    double* __restrict__ out) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const double q = ev_block_sum(t < nwg ? part[t] : 0.0, red);
  const double l = ev_block_sum(t < nwg ? part[EV_MAX_WGS + t] : 0.0, red);
  const double bad = ev_block_sum(t < nwg ? part[2 * EV_MAX_WGS + t] : 0.0, red);
  if (t == 0) {
    out[0] = *info < 0 ? ev_status_nan(EV_NAN_HANDOVER) : (bad > 0.0 ? ev_status_nan(EV_NAN_PADDING) : q);
    out[1] = 2.0 * l;
  }
}

// the identity panel: V (rows x cols, column-major, leading dimension rows) <- columns [0, cols) of the rows x rows identity
__global__ __launch_bounds__(EV_THREADS) void identity_panel_kernel(double* __restrict__ v, int64_t rows, int64_t cols) {
  const int64_t c = blockIdx.y + (int64_t)blockIdx.z * 65535;
  const int64_t r = (blockIdx.x * (int64_t)EV_THREADS + threadIdx.x) * 2;
  if (c >= cols || r >= rows) return;            // (rows is a multiple of 128: r + 1 < rows)
  *reinterpret_cast<double2*>(v + c * rows + r) = make_double2(r == c ? 1.0 : 0.0, r + 1 == c ? 1.0 : 0.0);
}

// out[c] = sum_{i >= c} V[i, c]^2  for the solved identity panel (column c is exactly zero above row c): one workgroup per column
__global__ __launch_bounds__(EV_THREADS) void col_sumsq_lower_kernel(const double* __restrict__ v, int64_t rows, int64_t cols, double* __restrict__ out) {
  __shared__ double red[4];
  const int64_t c = blockIdx.x + (int64_t)blockIdx.y * 65535;
  if (c >= cols) return;                         // (uniform over the workgroup)
  const double* col = v + c * rows;
  double acc = 0.0;
  for (int64_t i = (c & ~(int64_t)1) + 2 * threadIdx.x; i < rows; i += 2 * EV_THREADS) {
    const double2 x = *reinterpret_cast<const double2*>(col + i);
    acc = fma(x.x, x.x, acc);
    acc = fma(x.y, x.y, acc);
  }
  acc = ev_block_sum(acc, red);
  if (threadIdx.x == 0) out[c] = acc;
}

// The fused leave-one-out epilogue (eqs. 5.10 - 5.12 above), per padded row; out = [mean | var | logp], pn each.  The sum of
// logp over the LOGICAL rows: workgroup b adds its rows into part[b] (a padding row has d = 1, w = 0 and would add
// -1/2 log 2 pi: it is left out by its mark, and its three outputs are never gathered).
__global__ __launch_bounds__(EV_THREADS) void loo_epilogue_kernel(const double* __restrict__ w, const double* __restrict__ d, const double* __restrict__ y,
                                                                  const int32_t* __restrict__ lrow, int64_t pn, double* __restrict__ out,
                                                                  double* __restrict__ part) {
  __shared__ double red[4];
  double sum = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)EV_THREADS + threadIdx.x; i < pn; i += (int64_t)gridDim.x * EV_THREADS) {
    const double wi = w[i], di = d[i];
    const double var = 1.0 / di, step = wi * var;
    const double lp = 0.5 * log(di) - 0.5 * wi * step - 0.91893853320467274178;      // 1/2 log 2 pi
    out[i] = y[i] - step;
    out[pn + i] = var;
    out[2 * pn + i] = lp;
    if (lrow[i] >= 0) sum += lp;
  }
  sum = ev_block_sum(sum, red);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

__global__ __launch_bounds__(EV_THREADS) void loo_final_kernel(const double* __restrict__ part, int nwg, const int* __restrict__ info,
                                                               double* __restrict__ total) {
  __shared__ double red[4];
  const double s = ev_block_sum((int)threadIdx.x < nwg ? part[threadIdx.x] : 0.0, red);
  if (threadIdx.x == 0) *total = *info < 0 ? ev_status_nan(EV_NAN_HANDOVER) : s;
}

// workgroups of a stage-1 launch; max_wgs > 0 (the test hooks') caps them below what the size asks for
static int ev_wgs(int64_t pn, int max_wgs) {
  const int nwg = (int)std::min<int64_t>((pn + EV_THREADS - 1) / EV_THREADS, EV_MAX_WGS);
  return max_wgs > 0 ? std::min(nwg, max_wgs) : nwg;
}

static unsigned long long ev_bits(double v) {
  unsigned long long u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

static int ev_check_status(double v, const char* fn) {
  LPGP_CHECK(ev_bits(v) != EV_NAN_HANDOVER, "%s: resident single-vector solve: a hand-over between workgroups timed out; set LPGP_TRSV_RESIDENT=0", fn);
  LPGP_CHECK(ev_bits(v) != EV_NAN_PADDING, "%s: a padding row of the factor is not a row of the identity (or carries a residual)", fn);
  return 0;
}

// the host staging of a call: nvec logical vectors scattered into the padded layout (zeros in the padding rows), behind them the
// map padded row -> logical row (-1: padding) as pn int32
void ev_stage(const lpgp_mat* mat, const double* const* vecs, int nvec, std::vector<double>* h) {
  const int64_t pn = mat->pn;
  h->assign((size_t)(nvec * pn + (pn + 1) / 2), 0.0);
  int32_t* lrow = reinterpret_cast<int32_t*>(h->data() + (size_t)nvec * pn);
  std::fill(lrow, lrow + pn, -1);
  for (int k = 0; k < nvec; ++k) mat->scatter_padded(vecs[k], h->data() + (size_t)k * pn);
  mat->logical_of_padded(lrow);
}

int ev_upload(lpgp_ctx* ctx, double* dst, const std::vector<double>& h) {
  LPGP_HIP(hipMemcpyAsync(dst, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->s_main));
  ctx->evidence_h2d_bytes += (int64_t)(h.size() * sizeof(double));
  return 0;
}
int ev_download(lpgp_ctx* ctx, double* dst, const double* src, size_t doubles) {
  LPGP_HIP(hipMemcpyAsync(dst, src, doubles * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
  ctx->evidence_d2h_bytes += (int64_t)(doubles * sizeof(double));
  return 0;
}

// lpgp_mat_evidence: one forward solve of the residual through the single-vector path (trsv.hip), the two-stage reduction over
// the solved vector and the factor's diagonal, ONE read-back of 16 bytes.
int mat_evidence(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, double out_host[2], int max_wgs) {
  const int64_t pn = mat->pn, T = pn / TILE;
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  std::vector<double> h;
  ev_stage(mat, &r_host, 1, &h);
  // [r | lrow] as staged, z + the ticket word of the resident solve, the partials, the result
  const size_t o_z = h.size(), o_part = o_z + (size_t)pn + 2, o_out = o_part + 3 * EV_MAX_WGS;
  DevBuf buf;
  LPGP_TRY(DevBuf::pool(ctx, (o_out + 2) * sizeof(double), &buf));
  double* const d = buf.as();
  StreamDrain drain{st};                         // (the staging vector and the caller's array are borrowed by the copies)
  LPGP_TRY(ev_upload(ctx, d, h));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  if (ctx->trsv_resident) LPGP_TRY(solve_vec_fwd_resident(ctx, F, T, d, d + o_z, ctx->d_info));
  else LPGP_TRY(solve_vec_fwd(ctx, st, F, T, d, d + o_z));
  const int nwg = ev_wgs(pn, max_wgs);
  hipLaunchKernelGGL(evidence_partial_kernel, dim3((unsigned)nwg), dim3(EV_THREADS), 0, st, (const double*)(d + o_z), (const double*)mat->a, mat->lr_cap,
                     reinterpret_cast<const int32_t*>(d + pn), pn, d + o_part);
  hipLaunchKernelGGL(evidence_final_kernel, dim3(1), dim3(EV_THREADS), 0, st, (const double*)(d + o_part), nwg, (const int*)ctx->d_info, d + o_out);
  LPGP_HIP(hipGetLastError());
  LPGP_TRY(ev_download(ctx, out_host, d + o_out, 2));
  LPGP_TRY(drain.wait());
  return ev_check_status(out_host[0], "lpgp_mat_evidence");
}

// d_diag (pn doubles, device) <- diag(G^{-1}) in the padded layout, on the panel stream
int inverse_diag_device(lpgp_ctx* ctx, lpgp_mat* mat, double* d_diag) {
  const int64_t pn = mat->pn, panel = std::min<int64_t>(ctx->inverse_diag_panel, pn);
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  DevBuf vbuf;                                   // (reuse is ordered on the panel stream, which the blocked solve joins at its end)
  LPGP_TRY(DevBuf::pool(ctx, (size_t)pn * panel * sizeof(double), &vbuf));
  double* const v = vbuf.as();
  for (int64_t j0 = 0; j0 < pn; j0 += panel) {
    const int64_t rows = pn - j0, pc = std::min(panel, rows);
    const unsigned gy = (unsigned)(pc < 65535 ? pc : 65535), gz = (unsigned)((pc + 65534) / 65535);
    hipLaunchKernelGGL(identity_panel_kernel, dim3((unsigned)((rows / 2 + EV_THREADS - 1) / EV_THREADS), gy, gz), dim3(EV_THREADS), 0, st, v, rows, pc);
    LPGP_HIP(hipGetLastError());
    // against the trailing sub-factor L[j0:, j0:]
    LPGP_TRY(trsm_lower_blocked(ctx, F.trailing((int)(j0 / TILE)), rows / TILE, v, rows, pc));
    hipLaunchKernelGGL(col_sumsq_lower_kernel, dim3(gy, gz), dim3(EV_THREADS), 0, st, (const double*)v, rows, pc, d_diag + j0);
    LPGP_HIP(hipGetLastError());
  }
  return 0;
}

int mat_inverse_diag(lpgp_ctx* ctx, lpgp_mat* mat, double* out_host) {
  const int64_t pn = mat->pn;
  std::vector<double> h((size_t)pn);
  DevBuf dd;
  LPGP_TRY(DevBuf::pool(ctx, (size_t)pn * sizeof(double), &dd));
  StreamDrain drain{ctx->s_main};
  LPGP_TRY(inverse_diag_device(ctx, mat, dd.as()));
  LPGP_TRY(ev_download(ctx, h.data(), dd.as(), (size_t)pn));      // the n numbers, once, at the end
  LPGP_TRY(drain.wait());
  mat->gather_padded(h.data(), out_host);
  return 0;
}

// lpgp_mat_loo: w = G^{-1} r (single-vector solve), d = diag(G^{-1}) (above), the fused epilogue; logp_host[n] is the sum
int mat_loo(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, const double* y_host, double* mean_host, double* var_host, double* logp_host,
            int max_wgs) {
  const int64_t pn = mat->pn, n = mat->n, T = pn / TILE;
  hipStream_t st = ctx->s_main;
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  std::vector<double> h, res((size_t)(3 * pn + 1));
  const double* vecs[2] = {r_host, y_host};
  ev_stage(mat, vecs, 2, &h);
  // [w (r on entry) | y | lrow] as staged, the scratch of the solve (+ 2 ticket words), d, the partials, [mean | var | logp | sum]
  const size_t o_tmp = h.size(), o_d = o_tmp + (size_t)pn + 2, o_part = o_d + (size_t)pn, o_res = o_part + EV_MAX_WGS;
  DevBuf buf;
  LPGP_TRY(DevBuf::pool(ctx, (o_res + res.size()) * sizeof(double), &buf));
  double* const d = buf.as();
  const int32_t* lrow = reinterpret_cast<const int32_t*>(d + 2 * pn);
  StreamDrain drain{st};
  LPGP_TRY(ev_upload(ctx, d, h));
  LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  LPGP_TRY(solve_vec(ctx, F, T, d, d + o_tmp, ctx->d_info));
  LPGP_TRY(inverse_diag_device(ctx, mat, d + o_d));
  const int nwg = ev_wgs(pn, max_wgs);
  hipLaunchKernelGGL(loo_epilogue_kernel, dim3((unsigned)nwg), dim3(EV_THREADS), 0, st, (const double*)d, (const double*)(d + o_d), (const double*)(d + pn),
                     lrow, pn, d + o_res, d + o_part);
  hipLaunchKernelGGL(loo_final_kernel, dim3(1), dim3(EV_THREADS), 0, st, (const double*)(d + o_part), nwg, (const int*)ctx->d_info, d + o_res + 3 * pn);
  LPGP_HIP(hipGetLastError());
  LPGP_TRY(ev_download(ctx, res.data(), d + o_res, res.size()));
  LPGP_TRY(drain.wait());
  LPGP_TRY(ev_check_status(res[(size_t)(3 * pn)], "lpgp_mat_loo"));
  mat->gather_padded(res.data(), mean_host);
  mat->gather_padded(res.data() + pn, var_host);
  mat->gather_padded(res.data() + 2 * pn, logp_host);
  logp_host[n] = res[(size_t)(3 * pn)];
  return 0;
}

}  // namespace lpgp
