// Greedy pivoted Cholesky  G ~ L^T L  of a Gram OPERATOR, built and kept on the device.
//
// The algorithm is the one `randprocs/_matrix_free.PivotedCholeskyPreconditioner` states (the host loop there is its specification):
//   pivot    p = first index of the largest remaining diagonal entry d; stop at `rank`, at n, or at d[p] <= rtol * d0
//   row      g = row p of G, evaluated on the fly from one point against every block (the assembly kernels, unchanged)
//   commit   L[k] = (g + noise e_p - L[:k, p] @ L[:k]) / sqrt(d[p]);  d = max(d - L[k]^2, 0);  d[p] = 0
//   finish   delta = max(mean(d), delta_floor * d0);  S = delta I + L L^T  (rank x rank, to the host, which inverts it)
// The host drives the loop and reads 16 bytes per pivot; nothing of size rank x n crosses the bus.  Plain launches on the panel
// stream, no waiting between workgroups, no atomics: the same bits on every call.  The loop state and the column coverage of a
// row are kept by pivchol_state.h; nothing here writes those fields.
//
// Launch geometry (the tests put their sizes on its boundaries):
//   argmax    stage 1: min(ceil(n / 256), 256) workgroups of 256 threads, row i belongs to workgroup (i / 256) % G1 (grid-stride
//             trips of G1 * 256 rows); stage 2: one workgroup of 256 threads, one partial each.  Sum of d in the same pass:
//             depth ceil(n / 65 536) per thread + 8 + 8 tree levels.
//   commit    one thread per column, 256 per workgroup; the k values L[t, p] staged in LDS (LPGP_PIVCHOL_MAX_RANK doubles).
//             Roundings per entry: k fma, the square root, the division (+ 1 where the noise is added, j = p).
//   small Gram  one workgroup of 256 threads per entry of the lower triangle (the triangle folded into a rectangular grid, so
//             no workgroup is launched for the upper half): ceil(n / 256) fma per thread, 8 tree levels, the shift on the
//             diagonal; the entry is mirrored, so S == S^T bit for bit.  One stage per entry, not two: a whole workgroup has
//             only n / 256 rows per thread, and the order is fixed either way.  Every entry streams two rows of L (rank^2 n 8
//             bytes in all, 10 GB at rank 200 and n = 32 768, from cache); tiling rows of L is the follow-up.

#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "lpgp_internal.h"

namespace lpgp {

constexpr int PC_G1 = 256;         // most workgroups of the first argmax stage (== threads of the second)

struct PcBest {
  double v;
  long long i;
};
// the larger value; among equals the smaller index (np.argmax: the first)
__device__ __forceinline__ PcBest pc_better(PcBest a, PcBest b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

// 256-wide tree over (value, index), the sum and the NaN flag; the result in element 0 of each array
__device__ __forceinline__ void pc_tree(double* sv, long long* si, double* ss, int* sn) {
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const PcBest b = pc_better(PcBest{sv[threadIdx.x], si[threadIdx.x]}, PcBest{sv[threadIdx.x + o], si[threadIdx.x + o]});
      sv[threadIdx.x] = b.v;
      si[threadIdx.x] = b.i;
      ss[threadIdx.x] += ss[threadIdx.x + o];
      sn[threadIdx.x] |= sn[threadIdx.x + o];
    }
    __syncthreads();
  }
}
// part: [value G1 | index G1 (as int64 bits) | sum G1]; a NaN makes the workgroup's index -2
__global__ __launch_bounds__(256) void pivchol_argmax1_kernel(const double* __restrict__ d, int64_t n, double* __restrict__ part) {
  __shared__ double sv[256], ss[256];
  __shared__ long long si[256];
  __shared__ int sn[256];
  const int g = blockIdx.x, G = gridDim.x;
  PcBest best{-INFINITY, LLONG_MAX};
  double s = 0.0;
  int bad = 0;
  for (int64_t i = (int64_t)g * 256 + threadIdx.x; i < n; i += (int64_t)G * 256) {
    const double x = d[i];
    bad |= (x != x);
    if (x > best.v) best = PcBest{x, (long long)i};
    s += x;
  }
  sv[threadIdx.x] = best.v; si[threadIdx.x] = best.i; ss[threadIdx.x] = s; sn[threadIdx.x] = bad;
  __syncthreads();
  pc_tree(sv, si, ss, sn);
  if (threadIdx.x == 0) {
    part[g] = sv[0];
    reinterpret_cast<long long*>(part)[PC_G1 + g] = sn[0] ? -2 : si[0];
    part[2 * PC_G1 + g] = ss[0];
  }
}
// slot: {pivot (int64 bits; -2: NaN), d[pivot], sum}
__global__ __launch_bounds__(256) void pivchol_argmax2_kernel(const double* __restrict__ part, int G, double* __restrict__ slot) {
  __shared__ double sv[256], ss[256];
  __shared__ long long si[256];
  __shared__ int sn[256];
  const int t = threadIdx.x;
  const bool in = t < G;
  const long long idx = in ? reinterpret_cast<const long long*>(part)[PC_G1 + t] : LLONG_MAX;
  sv[t] = in ? part[t] : -INFINITY;
  si[t] = idx == -2 ? LLONG_MAX : idx;
  ss[t] = in ? part[2 * PC_G1 + t] : 0.0;
  sn[t] = idx == -2;
  __syncthreads();
  pc_tree(sv, si, ss, sn);
  if (t == 0) {
    reinterpret_cast<long long*>(slot)[0] = sn[0] ? -2 : si[0];
    slot[1] = sv[0];
    slot[2] = ss[0];
  }
}
// one[dim * 64 + i] = (i == 0) ? x[dim * n_pad + l] : 0: point l of a resident set as a set of its own
__global__ __launch_bounds__(256) void pivchol_gather_kernel(const double* __restrict__ x, int64_t n_pad, int d, int64_t l, double* __restrict__ one) {
  for (int e = threadIdx.x; e < d * 64; e += 256) one[e] = (e % 64 == 0) ? x[(int64_t)(e / 64) * n_pad + l] : 0.0;
}
// L[k, j] = (g_j + [j == p] noise_pp - sum_{t < k} L[t, p] L[t, j]) / sqrt(dp);  d[j] = max(d[j] - L[k, j]^2, 0);  d[p] = 0
__global__ __launch_bounds__(256) void pivchol_commit_kernel(double* __restrict__ L, double* __restrict__ d, const double* __restrict__ row2, int64_t n, int k,
                                                             int64_t p, double dp, double noise_pp) {
  __shared__ double lp[LPGP_PIVCHOL_MAX_RANK];
  for (int t = threadIdx.x; t < k; t += 256) lp[t] = L[(int64_t)t * n + p];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double s = row2[2 * j];
  if (j == p) s += noise_pp;
#pragma unroll 8
  for (int t = 0; t < k; ++t) s = fma(-lp[t], L[(int64_t)t * n + j], s);
  const double l = s / sqrt(dp);
  L[(int64_t)k * n + j] = l;
  d[j] = (j == p) ? 0.0 : fmax(d[j] - l * l, 0.0);
}
// S[a, b] = S[b, a] = <L[a], L[b]> (+ delta on the diagonal), a >= b
__global__ __launch_bounds__(256) void pivchol_gram_kernel(const double* __restrict__ L, int64_t n, int rank, double delta, double* __restrict__ S) {
  __shared__ double red[256];
  // the lower triangle folded into a (rank + 1) x ceil(rank / 2) grid: row y (y + 1 entries) beside row rank - 1 - y (rank - y entries)
  const int y = blockIdx.y, x = blockIdx.x;
  int a = y, b = x;
  if (x > y) {
    a = rank - 1 - y;
    b = x - y - 1;
    if (a == y) return;              // (odd rank: the middle row has no partner)
  }
  const double* la = L + (int64_t)a * n;
  const double* lb = L + (int64_t)b * n;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s = fma(la[i], lb[i], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double v = (a == b) ? red[0] + delta : red[0];
    S[(int64_t)a * rank + b] = v;
    S[(int64_t)b * rank + a] = v;
  }
}

// the two argmax stages on the panel stream, then slot[0 .. count) read back (waits)
static int pc_reduce(lpgp_pivchol* pc, int count, double* out) {
  hipStream_t st = pc->ctx->s_main;
  int64_t g1 = (pc->n + 255) / 256;
  if (g1 > PC_G1) g1 = PC_G1;
  hipLaunchKernelGGL(pivchol_argmax1_kernel, dim3((unsigned)g1), dim3(256), 0, st, (const double*)pc->d(), pc->n, pc->part());
  hipLaunchKernelGGL(pivchol_argmax2_kernel, dim3(1), dim3(256), 0, st, (const double*)pc->part(), (int)g1, pc->slot());
  LPGP_HIP(hipGetLastError());
  LPGP_HIP(hipMemcpyAsync(out, pc->slot(), (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
  LPGP_HIP(hipStreamSynchronize(st));
  return 0;
}
static int pc_pivot_of(const lpgp_pivchol* pc, const double* slot, const char* fn, int64_t* p) {
  long long idx;
  std::memcpy(&idx, slot, sizeof(idx));
  LPGP_CHECK(idx != -2, "%s: the remaining diagonal holds a NaN", fn);
  LPGP_CHECK(idx >= 0 && idx < pc->n, "%s: the remaining diagonal holds no finite entry", fn);
  *p = (int64_t)idx;
  return 0;
}

}  // namespace lpgp

using namespace lpgp;

#define LPGP_PIVCHOL_ENTRY(fn)                                                                                   \
  LPGP_CHECK(ctx && pc, fn ": null argument");                                                                   \
  LPGP_DEVICE(ctx);                                                                                              \
  LPGP_CHECK(!ctx->distributed(), fn ": single GPU only (this context has joined a multi-GPU job)");             \
  LPGP_CHECK(pc->ctx == ctx, fn ": the handle belongs to another context")

extern "C" {

int lpgp_pivchol_create(lpgp_ctx* ctx, int64_t n, int32_t max_rank, const double* diag_host, double rtol, lpgp_pivchol** out) {
  LPGP_CHECK(ctx && diag_host && out, "lpgp_pivchol_create: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "lpgp_pivchol_create: single GPU only (this context has joined a multi-GPU job)");
  LPGP_CHECK(n >= 1 && max_rank >= 0 && rtol >= 0.0, "lpgp_pivchol_create: n=%lld max_rank=%d rtol=%g", (long long)n, max_rank, rtol);
  LPGP_CHECK(max_rank <= LPGP_PIVCHOL_MAX_RANK, "lpgp_pivchol_create: rank %d above LPGP_PIVCHOL_MAX_RANK = %d (the commit kernel stages one column of L in LDS)",
             max_rank, LPGP_PIVCHOL_MAX_RANK);
  double d0 = diag_host[0];
  for (int64_t i = 1; i < n; ++i)
    if (diag_host[i] > d0) d0 = diag_host[i];       // (a NaN is found by the first pivot search, on the device)
  std::unique_ptr<lpgp_pivchol> pc(new lpgp_pivchol());
  pc->ctx = ctx;
  pc->init(n, max_rank, rtol, d0);
  pc->L_bytes = ((size_t)pc->max_rank * n + 8) * sizeof(double);
  pc->work_bytes = ((size_t)3 * n + LPGP_MAXD * 64 + 3 * PC_G1 + 8) * sizeof(double);
  DevBuf L, work;
  LPGP_TRY(DevBuf::pool(ctx, pc->L_bytes, &L));
  LPGP_TRY(DevBuf::pool(ctx, pc->work_bytes, &work));
  StreamDrain drain{ctx->s_main};                  // (the caller's diagonal is borrowed by the copy)
  LPGP_HIP(hipMemsetAsync(L.as(), 0, pc->L_bytes, ctx->s_main));
  LPGP_HIP(hipMemsetAsync(work.as(), 0, pc->work_bytes, ctx->s_main));
  LPGP_HIP(hipMemcpyAsync(work.as(), diag_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->s_main));
  LPGP_TRY(drain.wait());
  pc->L = (double*)L.release();
  pc->work = (double*)work.release();
  *out = pc.release();
  return 0;
}

int lpgp_pivchol_destroy(lpgp_pivchol* pc) {
  if (!pc) return 0;
  std::string err;
  if (const int rc = refused(pc->can_destroy(&err), err)) return rc;
  (void)hipSetDevice(pc->ctx->device);
  pool_free(pc->ctx, pc->L, pc->L_bytes);
  pool_free(pc->ctx, pc->work, pc->work_bytes);
  delete pc;
  return 0;
}

int lpgp_pivchol_pivot(lpgp_ctx* ctx, lpgp_pivchol* pc, int64_t* pivot, double* value) {
  LPGP_PIVCHOL_ENTRY("lpgp_pivchol_pivot");
  LPGP_CHECK(pivot && value, "lpgp_pivchol_pivot: null argument");
  std::string err;
  LPGP_TRY(refused(pc->can_pivot(&err), err));
  double slot[2];
  LPGP_TRY(pc_reduce(pc, 2, slot));
  int64_t p = -1;
  LPGP_TRY(pc_pivot_of(pc, slot, "lpgp_pivchol_pivot", &p));
  *value = slot[1];
  *pivot = pc->pivot_read(p, slot[1]);
  return 0;
}

int lpgp_pivchol_row(lpgp_ctx* ctx, lpgp_pivchol* pc, const lpgp_kdesc* kd, int32_t ngroups, const lpgp_pts* X_i, int64_t l, const lpgp_pts* X_j,
                     int64_t col_off) {
  LPGP_PIVCHOL_ENTRY("lpgp_pivchol_row");
  LPGP_CHECK(kd && X_i && X_j, "lpgp_pivchol_row: null argument");
  LPGP_CHECK(X_i->d == X_j->d && kd[0].d == X_i->d, "lpgp_pivchol_row: dimension mismatch");
  LPGP_CHECK(l >= 0 && l < X_i->n, "lpgp_pivchol_row: point %lld of a set of %lld", (long long)l, (long long)X_i->n);
  std::string err;
  LPGP_TRY(refused(pc->can_add_piece(col_off, X_j->n, &err), err));
  DevDesc desc;
  LPGP_TRY(lower_kdesc(kd, ngroups, &desc));
  if (X_j->n == 0) return 0;
  hipLaunchKernelGGL(pivchol_gather_kernel, dim3(1), dim3(256), 0, ctx->s_main, (const double*)X_i->x, X_i->n_pad, (int)X_i->d, l, pc->one());
  LPGP_HIP(hipGetLastError());
  // the call lpgp_kernel_matrix makes for one point against X_j: one row, leading dimension 2
  LPGP_TRY(launch_assemble(ctx, ctx->s_main, desc, pc->one(), 1, 64, X_j->x, X_j->n, X_j->n_pad, pc->row() + 2 * col_off, 2, 0, 0, 0));
  return refused(pc->add_piece(col_off, X_j->n, &err), err);
}

int lpgp_pivchol_commit(lpgp_ctx* ctx, lpgp_pivchol* pc, double noise_pp) {
  LPGP_PIVCHOL_ENTRY("lpgp_pivchol_commit");
  std::string err;
  LPGP_TRY(refused(pc->can_commit(&err), err));
  hipLaunchKernelGGL(pivchol_commit_kernel, dim3((unsigned)((pc->n + 255) / 256)), dim3(256), 0, ctx->s_main, pc->L, pc->d(), (const double*)pc->row(), pc->n,
                     (int)pc->rank, pc->pivot, pc->pivot_value, noise_pp);
  LPGP_HIP(hipGetLastError());
  return refused(pc->committed(&err), err);
}

int lpgp_pivchol_finish(lpgp_ctx* ctx, lpgp_pivchol* pc, double delta_floor, double* delta, double* S_host) {
  LPGP_PIVCHOL_ENTRY("lpgp_pivchol_finish");
  LPGP_CHECK(delta && (S_host || pc->rank == 0) && delta_floor >= 0.0, "lpgp_pivchol_finish: bad argument");
  std::string err;
  LPGP_TRY(refused(pc->can_finish(&err), err));
  double slot[3];
  LPGP_TRY(pc_reduce(pc, 3, slot));
  int64_t p = -1;
  LPGP_TRY(pc_pivot_of(pc, slot, "lpgp_pivchol_finish", &p));
  const double mean = slot[2] / (double)pc->n, floor = delta_floor * pc->d0;
  const double dl = mean > floor ? mean : floor;
  if (pc->rank > 0) {
    const size_t bytes = (size_t)pc->rank * pc->rank * sizeof(double);
    DevBuf S;
    LPGP_TRY(DevBuf::pool(ctx, bytes, &S));
    StreamDrain drain{ctx->s_main};                // (the caller's array is borrowed by the copy)
    hipLaunchKernelGGL(pivchol_gram_kernel, dim3((unsigned)pc->rank + 1, (unsigned)(pc->rank + 1) / 2), dim3(256), 0, ctx->s_main, (const double*)pc->L, pc->n, (int)pc->rank, dl,
                       S.as());
    LPGP_HIP(hipGetLastError());
    LPGP_HIP(hipMemcpyAsync(S_host, S.as(), bytes, hipMemcpyDeviceToHost, ctx->s_main));
    LPGP_TRY(drain.wait());
  }
  LPGP_TRY(refused(pc->finish(dl, &err), err));
  *delta = dl;
  return 0;
}

int lpgp_pivchol_info(const lpgp_pivchol* pc, int32_t* rank, double* d0, int64_t* pivots_host) {
  LPGP_CHECK(pc, "lpgp_pivchol_info: null argument");
  if (rank) *rank = pc->rank;
  if (d0) *d0 = pc->d0;
  if (pivots_host)
    for (size_t k = 0; k < pc->pivots.size(); ++k) pivots_host[k] = pc->pivots[k];
  return 0;
}

int lpgp_pivchol_to_host(lpgp_ctx* ctx, lpgp_pivchol* pc, int32_t what, double* out_host) {
  LPGP_PIVCHOL_ENTRY("lpgp_pivchol_to_host");
  LPGP_CHECK(out_host && what >= 0 && what <= 2, "lpgp_pivchol_to_host: bad argument (what = %d)", what);
  if (what == 0 && pc->rank == 0) return 0;
  std::vector<double> h;
  const double* src = what == 0 ? pc->L : what == 1 ? pc->d() : pc->row();
  const size_t count = what == 0 ? (size_t)pc->rank * pc->n : what == 1 ? (size_t)pc->n : (size_t)2 * pc->n;
  double* dst = out_host;
  if (what == 2) {
    h.resize(count);
    dst = h.data();
  }
  StreamDrain drain{ctx->s_main};
  LPGP_HIP(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
  LPGP_TRY(drain.wait());
  if (what == 2)
    for (int64_t j = 0; j < pc->n; ++j) out_host[j] = h[(size_t)2 * j];
  return 0;
}

}  // extern "C"
