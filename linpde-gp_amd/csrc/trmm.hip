// trmm.hip -- out = L Z for the lower Cholesky factor L of a factored lpgp_mat and a tall, narrow Z (n x s, s = 1 .. a few
// hundred): the product behind a joint draw  mean + C z  (lpgp_mat_factor_matmul; probnum `Normal.sample` / `cov_cholesky`).
//
// Roofline.  Every entry of the lower triangle of L is needed once: 4 n^2 bytes.  It meets s values of Z, i.e. 2 s flops per
// 8 bytes; at the 6.3 TB/s this device streams, s = 16 asks for 25 Tflop/s, a third of the fp64 vector rate -- so up to a
// column tile of TR_ST = 16 the product is bound by reading L, and plain fused multiply-adds with L in registers and Z
// broadcast from LDS reach that bound without the operand shuffles an MFMA fragment layout would need for a 16-wide B.  Wider
// Z is a loop over column tiles (grid dimension y): L is read again per tile, from L2 / the Infinity Cache while it fits.
//
// Work split.  Tile row i (128 rows) needs the tiles j <= i only -- a staircase.  It is cut into chunks of at most `kc` tiles
// of columns, one workgroup each, so that every workgroup streams about the same number of bytes whatever its row; the chunk
// size shrinks until the launch fills the device.  A workgroup's four waves split each 128-column tile four ways (32 columns
// each: one coalesced 1-KiB column segment per load, 16 bytes per lane = two rows), are summed through LDS in the order
// 0, 1, 2, 3, and the chunk's 128 x 16 partial goes to a scratch buffer.  A second kernel adds the chunks of a row in
// increasing order and the shift: no atomics, the same bits on every run.
//
// What is never read: tiles above the diagonal of the storage (a row's chunks stop at tile i), and inside the diagonal tile
// the entries above the diagonal are replaced by zeros whatever they hold.
#include <algorithm>
#include <cstring>

#include "lpgp_internal.h"

namespace lpgp {

constexpr int TR_ST = 16;          // columns of Z per pass
constexpr int TR_KC_MAX = 8;       // tiles of columns per workgroup at most (1 MiB of L)

__global__ __launch_bounds__(256) void trmm_lower_kernel(const double* __restrict__ L, int64_t ld, const double* __restrict__ Zt, int64_t pn,
                                                         const int32_t* __restrict__ wg_row, const int32_t* __restrict__ wg_j0, int kc,
                                                         double* __restrict__ part, int nct) {
  __shared__ double zs[2][TILE * TR_ST];          // the Z tile of the current / next 128 columns (double-buffered: one barrier per step)
  const int wg = blockIdx.x, ct = blockIdx.y;
  const int i = wg_row[wg], j0 = wg_j0[wg];
  const int j1 = min(j0 + kc, i + 1);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const double* zsrc = Zt + (int64_t)ct * pn * TR_ST;
  const double* lrow = L + (int64_t)i * TILE + 2 * lane;
  double acc0[TR_ST], acc1[TR_ST];
#pragma unroll
  for (int c = 0; c < TR_ST; ++c) acc0[c] = acc1[c] = 0.0;
  for (int j = j0; j < j1; ++j) {
    double* zb = zs[(j - j0) & 1];
    {
      const double2* src = reinterpret_cast<const double2*>(zsrc + (int64_t)j * TILE * TR_ST);
      double2* dst = reinterpret_cast<double2*>(zb);
#pragma unroll
      for (int q = 0; q < TILE * TR_ST / 2 / 256; ++q) dst[tid + 256 * q] = src[tid + 256 * q];
    }
    __syncthreads();
    const bool diag = (j == i);
    const int k0 = w * 32;
    const double* lp = lrow + ((int64_t)j * TILE + k0) * ld;
#pragma unroll 8
    for (int q = 0; q < 32; ++q) {
      double2 l = *reinterpret_cast<const double2*>(lp + (int64_t)q * ld);
      if (diag) {                                  // column k of the diagonal tile reaches the rows r >= k only
        if (k0 + q > 2 * lane) l.x = 0.0;
        if (k0 + q > 2 * lane + 1) l.y = 0.0;
      }
      const double* z = zb + (k0 + q) * TR_ST;
#pragma unroll
      for (int c = 0; c < TR_ST; ++c) {
        const double zc = z[c];
        acc0[c] = fma(l.x, zc, acc0[c]);
        acc1[c] = fma(l.y, zc, acc1[c]);
      }
    }
  }
  // waves 1, 2, 3 hand their sums to wave 0, one after the other (a fixed order of summation)
  double* red = &zs[0][0];                         // 128 x 16 doubles = one of the two Z buffers
  for (int ww = 1; ww < 4; ++ww) {
    __syncthreads();
    if (w == ww) {
#pragma unroll
      for (int c = 0; c < TR_ST; ++c) {
        red[(2 * lane) * TR_ST + c] = acc0[c];
        red[(2 * lane + 1) * TR_ST + c] = acc1[c];
      }
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int c = 0; c < TR_ST; ++c) {
        acc0[c] += red[(2 * lane) * TR_ST + c];
        acc1[c] += red[(2 * lane + 1) * TR_ST + c];
      }
    }
  }
  if (w == 0) {
    double* p = part + (((int64_t)wg * nct + ct) * TILE + 2 * lane) * TR_ST;
#pragma unroll
    for (int c = 0; c < TR_ST; ++c) {
      p[c] = acc0[c];
      p[TR_ST + c] = acc1[c];
    }
  }
}

// out[lrow[p], col] = shift[lrow[p]] + sum over the chunks of tile row p / 128, in increasing order
__global__ __launch_bounds__(256) void trmm_reduce_kernel(const double* __restrict__ part, const int32_t* __restrict__ lrow,
                                                          const int32_t* __restrict__ chunk0, int nct, int64_t s, int64_t pn,
                                                          const double* __restrict__ shift, double* __restrict__ out) {
  const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
  const int64_t per_row = (int64_t)nct * TR_ST;
  if (idx >= pn * per_row) return;
  const int64_t p = idx / per_row;
  const int rem = (int)(idx - p * per_row), ct = rem / TR_ST, c = rem % TR_ST;
  const int64_t col = (int64_t)ct * TR_ST + c;
  const int lr = lrow[p];
  if (col >= s || lr < 0) return;
  const int i = (int)(p / TILE), r = (int)(p % TILE);
  double sum = 0.0;
  for (int ch = chunk0[i]; ch < chunk0[i + 1]; ++ch) sum += part[(((int64_t)ch * nct + ct) * TILE + r) * TR_ST + c];
  out[(int64_t)lr * s + col] = (shift ? shift[lr] : 0.0) + sum;
}

int factor_matmul(lpgp_ctx* ctx, lpgp_mat* mat, const double* Z_host, int64_t s, const double* shift_host, double* out_host, int kc_force) {
  const int64_t pn = mat->pn, n = mat->n;
  const int T = (int)(pn / TILE), nct = (int)((s + TR_ST - 1) / TR_ST);
  LPGP_CHECK(nct <= 65535, "lpgp_mat_factor_matmul: at most %d columns", 65535 * TR_ST);
  // chunk size: as large as still fills the device twice over
  auto count_chunks = [&](int kc) { int64_t c = 0; for (int i = 0; i < T; ++i) c += (i + kc) / kc; return c; };
  int kc = TR_KC_MAX;
  const int64_t want = 2 * (int64_t)(ctx->cus > 0 ? ctx->cus : 256);
  while (kc > 1 && count_chunks(kc) * nct < want) kc /= 2;
  if (kc_force > 0) kc = kc_force;               // (the test hook's: any chunk size computes the same product)
  const int64_t nchunks = count_chunks(kc);
  // integer tables: [logical row of padded row p, or -1 | first chunk of tile row i (T + 1) | tile row of chunk | first tile of chunk]
  std::vector<int32_t> tab((size_t)(pn + T + 1 + 2 * nchunks), -1);
  mat->logical_of_padded(tab.data());
  int32_t* h_chunk0 = tab.data() + pn;
  int32_t* h_row = h_chunk0 + T + 1;
  int32_t* h_j0 = h_row + nchunks;
  {
    int32_t c = 0;
    for (int i = 0; i < T; ++i) {
      h_chunk0[i] = c;
      for (int j0 = 0; j0 <= i; j0 += kc, ++c) { h_row[c] = i; h_j0[c] = j0; }
    }
    h_chunk0[T] = c;
  }
  // Z as the kernel reads it: [column tile][padded row][16], zeros in the padding rows and columns; the shift behind it
  const size_t zdoubles = (size_t)nct * pn * TR_ST;
  std::vector<double> hz(zdoubles + (size_t)n, 0.0);
  for (int64_t p = 0; p < pn; ++p) {
    if (tab[(size_t)p] < 0) continue;
    const double* zr = Z_host + (int64_t)tab[(size_t)p] * s;
    for (int64_t c = 0; c < s; ++c) hz[((size_t)(c / TR_ST) * pn + (size_t)p) * TR_ST + (size_t)(c % TR_ST)] = zr[c];
  }
  if (shift_host) std::memcpy(hz.data() + zdoubles, shift_host, (size_t)n * sizeof(double));
  const size_t bz = hz.size() * sizeof(double), bt = tab.size() * sizeof(int32_t);
  const size_t bp = (size_t)nchunks * nct * TILE * TR_ST * sizeof(double), bo = (size_t)n * s * sizeof(double);
  DevBuf po, pp, pt, pz;                         // (declared in reverse: they go back into the pool in the order z, t, p, o)
  LPGP_TRY(DevBuf::pool(ctx, bz, &pz));
  LPGP_TRY(DevBuf::pool(ctx, bt, &pt));
  LPGP_TRY(DevBuf::pool(ctx, bp, &pp));
  LPGP_TRY(DevBuf::pool(ctx, bo, &po));
  hipStream_t st = ctx->s_main;
  StreamDrain drain{st};                         // (the staging vectors and the caller's array are borrowed by the copies)
  LPGP_HIP(hipMemcpyAsync(pz.as(), hz.data(), bz, hipMemcpyHostToDevice, st));
  LPGP_HIP(hipMemcpyAsync(pt.as(), tab.data(), bt, hipMemcpyHostToDevice, st));
  const int32_t* d_tab = pt.as<int32_t>();
  const double flops = (double)pn * (double)(pn + TILE) * (double)nct * TR_ST;
  prof_begin(ctx, st, LPGP_K_TRMM, flops, 4.0 * (double)pn * (double)(pn + TILE) * nct);
  hipLaunchKernelGGL(trmm_lower_kernel, dim3((unsigned)nchunks, (unsigned)nct), dim3(256), 0, st, (const double*)mat->a, mat->lr_cap,
                     (const double*)pz.as(), pn, d_tab + pn + T + 1, d_tab + pn + T + 1 + nchunks, kc, pp.as(), nct);
  LPGP_HIP(hipGetLastError());
  const int64_t total = pn * nct * TR_ST;
  hipLaunchKernelGGL(trmm_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)pp.as(), d_tab, d_tab + pn, nct, s, pn,
                     shift_host ? (const double*)pz.as() + zdoubles : (const double*)nullptr, po.as());
  LPGP_HIP(hipGetLastError());
  prof_end(ctx, st);
  LPGP_HIP(hipMemcpyAsync(out_host, po.as(), bo, hipMemcpyDeviceToHost, st));
  return drain.wait();
}

}  // namespace lpgp
