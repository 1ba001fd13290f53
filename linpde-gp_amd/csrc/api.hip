// C-ABI entry points of liblpgp.so (declared in include/lpgp.h).

#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <memory>

#include <rccl/rccl.h>

#include "lpgp_internal.h"
#include "mix_table.h"

namespace lpgp {

// ---------------------------------------------------------------------------------------
// profiling with HIP events on the launching stream
// ---------------------------------------------------------------------------------------
static hipEvent_t get_event(lpgp_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void prof_begin(lpgp_ctx* ctx, hipStream_t stream, int kernel, double flops, double bytes) {
  ctx->prof_open = 0;
  if (!(ctx->prof_on & (1 << kernel))) return;
  ctx->prof_open = 1;
  PendingEvent p;
  p.e0 = get_event(ctx);
  p.e1 = get_event(ctx);
  p.kernel = kernel;
  (void)hipEventRecord(p.e0, stream);
  ctx->pending.push_back(p);
  ctx->prof[kernel].launches += 1;
  ctx->prof[kernel].flops += flops;
  ctx->prof[kernel].bytes += bytes;
}

void prof_end(lpgp_ctx* ctx, hipStream_t stream) {
  if (!ctx->prof_open) return;
  ctx->prof_open = 0;
  (void)hipEventRecord(ctx->pending.back().e1, stream);
}

int prof_collect(lpgp_ctx* ctx) {
  if (ctx->pending.empty()) return 0;
  LPGP_HIP(hipDeviceSynchronize());
  for (auto& p : ctx->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) ctx->prof[p.kernel].ms += ms;
    ctx->event_pool.push_back(p.e0);
    ctx->event_pool.push_back(p.e1);
  }
  ctx->pending.clear();
  return 0;
}

// ---------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------
__global__ void set_identity_kernel(double* a, int64_t ld, int64_t from, int64_t to, Layout2D lay) {
  int64_t i = from + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= to) return;
  const int64_t lr = cyc_local(lay.rows, i), lc = cyc_local(lay.cols, i);
  if (lr >= 0 && lc >= 0) a[lr + lc * ld] = 1.0;
}

// out[j] = sum_i K[i + j*ld] * (w ? w[i] : K[i + j*ld])   over i < rows; one block per column
__global__ __launch_bounds__(256) void col_reduce_kernel(const double* __restrict__ K, int64_t ld, int64_t rows,
                                                          const double* __restrict__ w, double* __restrict__ out) {
  __shared__ double red[4];
  const double* col = K + (int64_t)blockIdx.x * ld;
  double acc = 0.0;
  for (int64_t i = threadIdx.x * 2; i < rows; i += 512) {
    double2 v = *reinterpret_cast<const double2*>(col + i);
    if (w) {
      double2 ww = *reinterpret_cast<const double2*>(w + i);
      acc = fma(v.x, ww.x, acc);
      acc = fma(v.y, ww.y, acc);
    } else {
      acc = fma(v.x, v.x, acc);
      acc = fma(v.y, v.y, acc);
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// both read-outs of the solved cross-covariance V = L^{-1} K in one pass:
//   out_dot[j] = sum_i V[i,j] z[i]   (posterior mean term  K_xX G^{-1} r = V^T z,  z = L^{-1} r)
//   out_sq[j]  = sum_i V[i,j]^2      (variance reduction)
__global__ __launch_bounds__(256) void col_reduce2_kernel(const double* __restrict__ V, int64_t ld, int64_t rows,
                                                           const double* __restrict__ z, double* __restrict__ out_dot,
                                                           double* __restrict__ out_sq) {
  __shared__ double red[8];
  const double* col = V + (int64_t)blockIdx.x * ld;
  double ad = 0.0, as = 0.0;
  for (int64_t i = threadIdx.x * 2; i < rows; i += 512) {
    const double2 v = *reinterpret_cast<const double2*>(col + i);
    const double2 zz = *reinterpret_cast<const double2*>(z + i);
    ad = fma(v.x, zz.x, ad);
    ad = fma(v.y, zz.y, ad);
    as = fma(v.x, v.x, as);
    as = fma(v.y, v.y, as);
  }
  for (int off = 32; off > 0; off >>= 1) {
    ad += __shfl_down(ad, off);
    as += __shfl_down(as, off);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = ad;
    red[4 + (threadIdx.x >> 6)] = as;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out_dot[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    out_sq[blockIdx.x] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

// the fill mode of the test hook (ctx->pool_fill >= 0): on the panel stream, where the reuse of a pool buffer is ordered -- a first
// use on another stream that does not wait for the panel stream is overtaken by the fill, and shows
static int pool_fill_buffer(lpgp_ctx* ctx, void* p, size_t bytes) {
  LPGP_HIP(hipMemsetAsync(p, ctx->pool_fill, bytes, ctx->s_main));
  ctx->pool_filled[0] += 1;
  ctx->pool_filled[1] += (int64_t)bytes;
  return 0;
}

int pool_alloc(lpgp_ctx* ctx, void** out, size_t bytes, bool* fresh) {
  int best = -1;
  for (int i = 0; i < (int)ctx->pool.size(); ++i) {
    const auto& b = ctx->pool[i];
    // (slack of half the request + 64 KB: with 1 MB, an 18-KB request took the 1.2-MB buffer of the tile inverses of a small matrix,
    //  whose own request then went to hipMalloc, and the overflowing pool to hipFree -- 0.18 ms per step at N_tot = 1 152)
    if (b.bytes >= bytes && b.bytes <= bytes + bytes / 2 + (64 << 10) && (best < 0 || b.bytes < ctx->pool[best].bytes)) best = i;
  }
  if (best >= 0) {
    const lpgp_ctx::PoolBuf taken = ctx->pool[best];
    *out = taken.p;
    ctx->pool.erase(ctx->pool.begin() + best);
    if (fresh) *fresh = false;
    if (ctx->pool_fill >= 0 && pool_fill_buffer(ctx, taken.p, bytes) != 0) {
      ctx->pool.push_back(taken);              // (nobody owns it yet: back where it came from)
      *out = nullptr;
      return -1;
    }
    return 0;
  }
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) {
    // release cached buffers and retry once
    for (auto& b : ctx->pool) (void)hipFree(b.p);
    ctx->pool.clear();
    e = hipMalloc(out, bytes);
  }
  if (e != hipSuccess) {
    set_error("device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return -1;
  }
  if (fresh) *fresh = true;
  if (ctx->pool_fill >= 0 && pool_fill_buffer(ctx, *out, bytes) != 0) {
    (void)hipFree(*out);
    *out = nullptr;
    return -1;
  }
  return 0;
}

void pool_free(lpgp_ctx* ctx, void* p, size_t bytes) {
  if (!p) return;
  if (ctx->pool.size() >= 12) {
    // drop the smallest cached buffer
    int sm = 0;
    for (int i = 1; i < (int)ctx->pool.size(); ++i)
      if (ctx->pool[i].bytes < ctx->pool[sm].bytes) sm = i;
    (void)hipFree(ctx->pool[sm].p);
    ctx->pool.erase(ctx->pool.begin() + sm);
  }
  ctx->pool.push_back({p, bytes});
}

__global__ void clear_rows_kernel(double* a, int64_t ld, int64_t r0, int64_t nr, int64_t c0, int64_t nc, Layout2D lay) {
  // zero the strip rows [r0, r0+nr) x cols [c0, c0+nc) of the GLOBAL padded matrix (the part this rank owns)
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t c = blockIdx.y + (int64_t)blockIdx.z * 65535;
  if (i >= nr || c >= nc) return;
  const int64_t lr = cyc_local(lay.rows, r0 + i), lc = cyc_local(lay.cols, c0 + c);
  if (lr >= 0 && lc >= 0) a[lr + lc * ld] = 0.0;
}
// identity tail of a block in ONE launch (round 5; three launches until then: a chain of small conditionings is launch-bound):
// pad rows [r0, r0 + pad) x columns [0, r0) <- 0;  rows [r0, cap) x pad columns [r0, r0 + pad) <- 0, ones on the diagonal
__global__ void pad_block_kernel(double* a, int64_t ld, int64_t r0, int64_t pad, int64_t cap, Layout2D lay) {
  const int64_t c = blockIdx.y + (int64_t)blockIdx.z * 65535;          // columns [0, r0 + pad)
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= r0 + pad) return;
  const int64_t row = r0 + i;
  if (row >= (c < r0 ? r0 + pad : cap)) return;
  const int64_t lr = cyc_local(lay.rows, row), lc = cyc_local(lay.cols, c);
  if (lr >= 0 && lc >= 0) a[lr + lc * ld] = (row == c) ? 1.0 : 0.0;
}
static void launch_pad_block(hipStream_t st, double* a, int64_t ld, int64_t r0, int64_t pad, int64_t cap, const Layout2D& lay) {
  const int64_t nc = r0 + pad, nr = cap - r0;
  const unsigned gy = (unsigned)(nc < 65535 ? nc : 65535), gz = (unsigned)((nc + 65534) / 65535);
  hipLaunchKernelGGL(pad_block_kernel, dim3((unsigned)((nr + 255) / 256), gy, gz), dim3(256), 0, st, a, ld, r0, pad, cap, lay);
}
// ... and, for lpgp_mat_condition, together with the block's measurement noise on the diagonal (sigma^2 I or a vector): ONE launch
// behind the assembly instead of a padding launch in front of it and an add_diag launch behind it.  The padding is the
// arithmetic of pad_block_kernel, the noise that of add_diag_kernel (one addition per diagonal entry: identical bits).
__global__ void finish_block_kernel(double* a, int64_t ld, int64_t r0, int64_t pad, int64_t cap, Layout2D lay, int64_t ncols, int64_t d0, int64_t dn,
                                    const double* dv, double dscalar) {
  const int64_t c = blockIdx.y + (int64_t)blockIdx.z * 65535;          // columns [0, ncols): padding; slice ncols: the noise
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c == ncols) {
    if (i < dn) {
      const int64_t lr = cyc_local(lay.rows, d0 + i), lc = cyc_local(lay.cols, d0 + i);
      if (lr >= 0 && lc >= 0) a[lr + lc * ld] += (dv ? dv[i] : 0.0) + dscalar;
    }
    return;
  }
  if (c > ncols) return;
  const int64_t row = r0 + i;
  if (row >= (c < r0 ? r0 + pad : cap)) return;
  const int64_t lr = cyc_local(lay.rows, row), lc = cyc_local(lay.cols, c);
  if (lr >= 0 && lc >= 0) a[lr + lc * ld] = (row == c) ? 1.0 : 0.0;
}
// pad == 0: noise only; dn == 0: padding only
static void launch_finish_block(hipStream_t st, double* a, int64_t ld, int64_t r0, int64_t pad, int64_t cap, const Layout2D& lay, int64_t d0, int64_t dn,
                                const double* dv, double dscalar) {
  const int64_t ncols = pad > 0 ? r0 + pad : 0, nr = pad > 0 ? cap - r0 : 0;
  if (ncols == 0 && dn == 0) return;
  const int64_t rows = nr > dn ? nr : dn, slices = ncols + (dn > 0 ? 1 : 0);
  const unsigned gy = (unsigned)(slices < 65535 ? slices : 65535), gz = (unsigned)((slices + 65534) / 65535);
  hipLaunchKernelGGL(finish_block_kernel, dim3((unsigned)((rows + 255) / 256), gy, gz), dim3(256), 0, st, a, ld, r0, pad, cap, lay, ncols, d0, dn, dv,
                     dscalar);
}
static void launch_clear_rows(hipStream_t st, double* a, int64_t ld, int64_t r0, int64_t nr, int64_t c0, int64_t nc, const Layout2D& lay) {
  if (nr <= 0 || nc <= 0) return;
  const unsigned gy = (unsigned)(nc < 65535 ? nc : 65535), gz = (unsigned)((nc + 65534) / 65535);
  hipLaunchKernelGGL(clear_rows_kernel, dim3((unsigned)((nr + 255) / 256), gy, gz), dim3(256), 0, st, a, ld, r0, nr, c0, nc, lay);
}

static int ensure_tmp(lpgp_ctx* ctx, int64_t n) {
  if (n <= ctx->tmp_cap) return 0;
  if (ctx->d_tmp) LPGP_HIP(hipFree(ctx->d_tmp));
  ctx->d_tmp = nullptr;
  ctx->tmp_cap = 0;
  LPGP_HIP(hipMalloc(&ctx->d_tmp, (size_t)n * sizeof(double)));
  ctx->tmp_cap = n;
  if (ctx->pool_fill >= 0) LPGP_TRY(pool_fill_buffer(ctx, ctx->d_tmp, (size_t)n * sizeof(double)));
  return 0;
}

static int ensure_stage(lpgp_ctx* ctx, int64_t n) {
  if (n <= ctx->stage_cap) return 0;
  if (ctx->h_stage) LPGP_HIP(hipHostFree(ctx->h_stage));
  ctx->h_stage = nullptr;
  ctx->stage_cap = 0;
  LPGP_HIP(hipHostMalloc(&ctx->h_stage, (size_t)n * sizeof(double), hipHostMallocDefault));
  ctx->stage_cap = n;
  return 0;
}

// layout of the matrix of this context: identity on a single GPU, the rank's share of the Pr x Pc grid otherwise
static Layout2D mat_layout(const lpgp_ctx* ctx) { return ctx->distributed() ? ctx->layout() : Layout2D(); }
static int64_t local_rows(const lpgp_ctx* ctx, int64_t padded) { return (int64_t)cyc_before(mat_layout(ctx).rows, (int)(padded / TILE)) * TILE; }
static int64_t local_cols(const lpgp_ctx* ctx, int64_t padded) { return (int64_t)cyc_before(mat_layout(ctx).cols, (int)(padded / TILE)) * TILE; }

static size_t mat_bytes_a(const lpgp_mat* m) { return (size_t)m->lr_cap * m->lc_cap * sizeof(double); }
static size_t mat_bytes_l(int64_t cap) { return (size_t)cap * TILE * sizeof(double); }
static size_t mat_bytes_w(int64_t cap) { return (size_t)(2 * cap + 8) * sizeof(double); }   // w | r | status word of the enqueued factorisations (lpgp_mat::d_status)
static size_t mat_bytes_d(const lpgp_ctx* ctx, int64_t cap) { return (size_t)round_up(cap, ctx->nb) * ctx->nb * sizeof(double); }

static void mat_release(lpgp_ctx* ctx, lpgp_mat* mat) {
  pool_free(ctx, mat->a, mat_bytes_a(mat));
  pool_free(ctx, mat->linv, mat_bytes_l(mat->cap));
  pool_free(ctx, mat->w, mat_bytes_w(mat->cap));
  if (mat->dblk) pool_free(ctx, mat->dblk, mat_bytes_d(ctx, mat->cap));
  mat->a = mat->linv = mat->w = mat->dblk = nullptr;
}

static int mat_alloc(lpgp_ctx* ctx, lpgp_mat* mat, int64_t cap) {
  // (re)allocate to `cap` (multiple of TILE) keeping the content of the first mat->pn rows/cols (of this rank's
  // share: the local index of a tile does not depend on the capacity).
  // Invariant kept for every buffer handed out: nothing is assumed about the lower triangle
  // of logical blocks (assembly overwrites it) nor about tiles above the diagonal (never
  // read); the padding strips of a block are cleared in lpgp_mat_add_block.
  const Layout2D lay = mat_layout(ctx);
  int64_t lr = local_rows(ctx, cap), lc = local_cols(ctx, cap);
  if (lr < TILE) lr = TILE;
  if (lc < TILE) lc = TILE;
  lpgp_mat fresh_dims;
  fresh_dims.lr_cap = lr; fresh_dims.lc_cap = lc;
  DevBuf ba, bl, bw, bd;
  LPGP_TRY(DevBuf::pool(ctx, mat_bytes_a(&fresh_dims), &ba));
  LPGP_TRY(DevBuf::pool(ctx, mat_bytes_l(cap), &bl));
  LPGP_TRY(DevBuf::pool(ctx, mat_bytes_w(cap), &bw));
  if (ctx->distributed()) LPGP_TRY(DevBuf::pool(ctx, mat_bytes_d(ctx, cap), &bd));
  double *const na = ba.as(), *const nl = bl.as(), *const nw = bw.as(), *const nd = bd.as();
  const int64_t pn_all = mat->padded_end(mat->total_blocks());
  if (mat->a && pn_all > 0) {
    const int64_t lru = local_rows(ctx, pn_all), lcu = local_cols(ctx, pn_all);
    if (lru > 0 && lcu > 0)
      LPGP_HIP(hipMemcpy2DAsync(na, (size_t)lr * sizeof(double), mat->a, (size_t)mat->lr_cap * sizeof(double),
                                (size_t)lru * sizeof(double), (size_t)lcu, hipMemcpyDeviceToDevice, ctx->s_main));
    LPGP_HIP(hipMemcpyAsync(nl, mat->linv, (size_t)pn_all * TILE * sizeof(double), hipMemcpyDeviceToDevice,
                            ctx->s_main));
    LPGP_HIP(hipMemcpyAsync(nw, mat->w, (size_t)pn_all * sizeof(double), hipMemcpyDeviceToDevice, ctx->s_main));
    LPGP_HIP(hipMemcpyAsync((double*)nw + 2 * cap, mat->d_status, sizeof(double), hipMemcpyDeviceToDevice, ctx->s_main));   // (sticky status: kept)
    if (nd) LPGP_HIP(hipMemcpyAsync(nd, mat->dblk, mat_bytes_d(ctx, pn_all), hipMemcpyDeviceToDevice, ctx->s_main));
    // padding columns of the existing blocks must stay zero in the rows added by the growth
    for (const auto& b : mat->blocks) {
      const int64_t padc = b.pn - b.n;
      if (padc > 0) launch_clear_rows(ctx->s_main, (double*)na, lr, pn_all, cap - pn_all, b.poff + b.n, padc, lay);
    }
  }
  if (!(mat->a && pn_all > 0)) LPGP_HIP(hipMemsetAsync((double*)nw + 2 * cap, 0, sizeof(double), ctx->s_main));       // a new / empty matrix: status clear
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));
  if (mat->a) mat_release(ctx, mat);
  mat->a = (double*)ba.release();
  mat->linv = (double*)bl.release();
  mat->w = (double*)bw.release();
  mat->d_status = reinterpret_cast<int*>(mat->w + 2 * cap);
  mat->dblk = (double*)bd.release();
  mat->cap = cap;
  mat->lr_cap = lr;
  mat->lc_cap = lc;
  mat->storage_moved();
  return 0;
}

}  // namespace lpgp

using namespace lpgp;

extern "C" {

const char* lpgp_last_error(void) { return lpgp::last_error(); }

int lpgp_init(int device, lpgp_ctx** out) {
  LPGP_CHECK(out != nullptr, "lpgp_init: null out");
  int ndev = 0;
  LPGP_HIP(hipGetDeviceCount(&ndev));
  LPGP_CHECK(ndev > 0, "lpgp_init: no HIP device visible (this library has no CPU fallback)");
  LPGP_CHECK(device >= 0 && device < ndev, "lpgp_init: device %d out of range (%d visible)", device, ndev);
  LPGP_HIP(hipSetDevice(device));
  lpgp_ctx* ctx = new lpgp_ctx();
  ctx->device = device;
  options_from_env(*ctx);
  hipDeviceProp_t prop;
  LPGP_HIP(hipGetDeviceProperties(&prop, device));
  ctx->cus = prop.multiProcessorCount;
  int lo = 0, hi = 0;
  LPGP_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
  LPGP_HIP(hipStreamCreateWithPriority(&ctx->s_main, hipStreamNonBlocking, hi));
  // The trailing-update stream may use all CUs except a few reserved ones, so that the
  // panel kernels of the look-ahead (a 156-KB-LDS tile Cholesky needs a whole CU) never queue
  // behind thousands of resident update workgroups.  reserve_cus = 0 (LPGP_RESERVE_CUS=0) disables the mask.
  // 32 = four CUs per XCD.  In steady state the mask costs the rank-512 update 10 % whether 1, 8 or 32 CUs are missing (65.1 ->
  // 58.8 / 58.5 TFLOP/s: the dispatcher feeds the shader engines evenly, so the first missing CU of an engine already sets
  // its pace; 64 missing cost 22 %; profiles/r03_clock_power.txt) -- so the chain may as well have the 32: c3 55.03-55.21 ms
  // against 55.18-55.64 with 8, c2 / c4 / c5 within their spread (MEASUREMENTS.md).
  // mask bit i = CU (i / 8) of XCD (i % 8) (measured, scratch/cumask.hip): clearing the low
  // `reserve_cus` bits takes the CUs round-robin from the XCDs, reserve_cus / 8 per XCD,
  // so a single workgroup of the panel stream finds a free CU on whichever XCD it is dealt to
  auto masked_stream = [&](int nreserve, hipStream_t* out) {
    *out = nullptr;
    if (nreserve == 0 || nreserve >= ctx->cus) return;       // (negative: a CU-masked queue with every CU enabled, for measurements)
    const int words = (ctx->cus + 31) / 32;
    std::vector<uint32_t> mask(words, 0u);
    for (int cu = 0; cu < ctx->cus; ++cu) mask[cu / 32] |= (1u << (cu % 32));
    for (int r = 0; r < nreserve; ++r) mask[r / 32] &= ~(1u << (r % 32));
    if (hipExtStreamCreateWithCUMask(out, (uint32_t)words, mask.data()) != hipSuccess) {
      (void)hipGetLastError();
      *out = nullptr;
    }
  };
  // single_stream (LPGP_SINGLE_STREAM=1): every stream of the context is the panel stream (no concurrency between chain and update).  For
  // jobs whose ranks SHARE one GPU (tests: eight processes x six queues oversubscribe the device's hardware queues and a
  // small eight-rank case takes 300 s; with one queue per process it takes a fraction of that).  Never a production setting.
  if (ctx->single_stream) {
    ctx->s_upd = ctx->s_upd_narrow = ctx->s_upd_all = ctx->s_outer = ctx->s_main;
  } else {
  masked_stream(ctx->reserve_cus, &ctx->s_upd);
  if (!ctx->s_upd) LPGP_HIP(hipStreamCreateWithPriority(&ctx->s_upd, hipStreamNonBlocking, lo));
  // While the panel chain bounds the pipeline (small trailing matrix) the update can spare a
  // quarter of the chip: with only 8 reserved CUs the chain's TRSM / in-panel update wait for
  // update workgroups to retire (measured at panel 20 of c3: 92 + 154 us instead of 21 + 15).
  masked_stream(ctx->reserve_narrow, &ctx->s_upd_narrow);
  // (a CU mask costs more than its CUs: a 16384^2 x 512 SYRK runs at 53.5 TFLOP/s unmasked, 49.4
  //  with 8 CUs removed (tile-count quantisation on 496 instead of 512 slots), 44.3 with 64
  //  removed; LPGP_TEST_GEMM_STREAM + scratch/gemm_sweep.py.  Only the factorisation needs it.)
  LPGP_HIP(hipStreamCreateWithPriority(&ctx->s_upd_all, hipStreamNonBlocking, lo));
  masked_stream(ctx->reserve_cus, &ctx->s_outer);
  if (!ctx->s_outer) LPGP_HIP(hipStreamCreateWithPriority(&ctx->s_outer, hipStreamNonBlocking, lo));
  }
  for (int i = 0; i < 2; ++i) {
    LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_outer[i], hipEventDisableTiming));
    LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_outer_fact[i], hipEventDisableTiming));
    LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_outer_a1[i], hipEventDisableTiming));
  }
  for (int i = 0; i < 4; ++i) LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_ride[i], hipEventDisableTiming));
  LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_chain_pre, hipEventDisableTiming));
  LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_chain_rows, hipEventDisableTiming));
  LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_append[0], hipEventDisableTiming));
  LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_append[1], hipEventDisableTiming));
  for (int i = 0; i < 2; ++i) {
    LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_panel[i], hipEventDisableTiming));
    LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_upd[i], hipEventDisableTiming));
  }
  for (auto& sl : ctx->desc_ring) {
    LPGP_HIP(hipHostMalloc(&sl.h, sizeof(DevDesc), hipHostMallocDefault));
    LPGP_HIP(hipMalloc(&sl.d, sizeof(DevDesc)));
    LPGP_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
  }
  LPGP_HIP(hipMalloc(&ctx->d_info, sizeof(int)));
  LPGP_HIP(hipHostMalloc(&ctx->h_info_pinned, 64, hipHostMallocDefault));
  *out = ctx;
  return 0;
}

int lpgp_finalize(lpgp_ctx* ctx) {
  if (!ctx) return 0;
  (void)hipSetDevice(ctx->device);
  if (ctx->nccl_comm && ctx->world > 1 && sync_stream(ctx, ctx->s_main) != 0) {
    // (sync_stream has aborted the communicators: a kernel of this rank was still waiting for a peer that is gone)
  }
  (void)hipDeviceSynchronize();
  for (auto& p : ctx->pending) {
    (void)hipEventDestroy(p.e0);
    (void)hipEventDestroy(p.e1);
  }
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ctx->ev_ride[i]);
  (void)hipEventDestroy(ctx->ev_chain_pre);
  if (ctx->ev_chain_rows) (void)hipEventDestroy(ctx->ev_chain_rows);
  for (auto& e : ctx->ev_append) if (e) (void)hipEventDestroy(e);
  for (int i = 0; i < 2; ++i) {
    (void)hipEventDestroy(ctx->ev_panel[i]);
    (void)hipEventDestroy(ctx->ev_upd[i]);
    (void)hipEventDestroy(ctx->ev_outer[i]);
    (void)hipEventDestroy(ctx->ev_outer_fact[i]);
    (void)hipEventDestroy(ctx->ev_outer_a1[i]);
  }
  for (auto& sl : ctx->desc_ring) {
    (void)hipHostFree(sl.h);
    (void)hipFree(sl.d);
    (void)hipEventDestroy(sl.done);
  }
  (void)hipFree(ctx->d_info);
  if (ctx->d_chain_flags) (void)hipFree(ctx->d_chain_flags);
  (void)hipHostFree(ctx->h_info_pinned);
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  for (auto& b : ctx->pts_pool) (void)hipFree(b.p);
  ctx->pts_pool.clear();
  for (auto& sl : ctx->pts_ring) {
    if (sl.h) (void)hipHostFree(sl.h);
    if (sl.done) (void)hipEventDestroy(sl.done);
  }
  if (ctx->h_stage_r) (void)hipHostFree(ctx->h_stage_r);
  if (ctx->ev_stage_r) (void)hipEventDestroy(ctx->ev_stage_r);
  if (ctx->d_tmp) (void)hipFree(ctx->d_tmp);
  for (size_t r = 0; r < ctx->ipc_peer.size(); ++r)
    if ((int)r != ctx->rank && ctx->ipc_peer[r]) (void)hipIpcCloseMemHandle(ctx->ipc_peer[r]);
  if (ctx->ipc_window) (void)hipFree(ctx->ipc_window);
  for (int i = 0; i < 2; ++i)
    if (ctx->ev_ipc[i]) (void)hipEventDestroy(ctx->ev_ipc[i]);
  if (ctx->d_pack) (void)hipFree(ctx->d_pack);
  for (int i = 0; i < 2; ++i)
    if (ctx->d_panel[i]) (void)hipFree(ctx->d_panel[i]);
  if (ctx->nccl_comm_bulk) (void)ncclCommDestroy((ncclComm_t)ctx->nccl_comm_bulk);
  if (ctx->nccl_comm) (void)ncclCommDestroy((ncclComm_t)ctx->nccl_comm);
  if (ctx->d_pack_bulk) (void)hipFree(ctx->d_pack_bulk);
  if (ctx->s_comm) (void)hipStreamDestroy(ctx->s_comm);
  for (int i = 0; i < 2; ++i) {
    if (ctx->ev_tail[i]) (void)hipEventDestroy(ctx->ev_tail[i]);
    if (ctx->ev_rows[i]) (void)hipEventDestroy(ctx->ev_rows[i]);
  }
  for (auto& b : ctx->pool) (void)hipFree(b.p);
  ctx->pool.clear();
  if (!ctx->single_stream) {
    (void)hipStreamDestroy(ctx->s_upd);
    if (ctx->s_upd_narrow) (void)hipStreamDestroy(ctx->s_upd_narrow);
    (void)hipStreamDestroy(ctx->s_upd_all);
    if (ctx->s_outer) (void)hipStreamDestroy(ctx->s_outer);
  }
  (void)hipStreamDestroy(ctx->s_main);
  delete ctx;
  return 0;
}

int lpgp_device_info(lpgp_ctx* ctx, char* name, int len, int* cus, int64_t* hbm_bytes) {
  LPGP_DEVICE(ctx);
  hipDeviceProp_t prop;
  LPGP_HIP(hipGetDeviceProperties(&prop, ctx->device));
  if (name && len > 0) {
    std::snprintf(name, (size_t)len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (cus) *cus = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
  return 0;
}

int lpgp_sync(lpgp_ctx* ctx) {
  LPGP_HIP(hipSetDevice(ctx->device));
  LPGP_HIP(hipDeviceSynchronize());
  return 0;
}

// read-only state beside the options: the matrices alive and the route counters (lpgp_ctx::RouteCounts)
#define ROUTE(name) {"route_" #name, &lpgp_ctx::RouteCounts::name}
static const struct { const char* key; int64_t lpgp_ctx::RouteCounts::*count; } kRoutes[] = {
    ROUTE(ride_done), ROUTE(ride_aug), ROUTE(ride_b2b), ROUTE(ride), ROUTE(ride_vchain), ROUTE(ride_two), ROUTE(ride_outer),
    ROUTE(solve_two_level), ROUTE(solve_ahead), ROUTE(solve_tiles)};
#undef ROUTE
// the context state of evidence.hip and evidence_cv.hip, beside the option table like the rows above: the panel width of the inverse
// diagonal and the fold batch of the cross-validation (the two keys of these that lpgp_set_option takes), the byte counters of their copies
static const struct { const char* key; int64_t lpgp_ctx::*field; } kEvidence[] = {
    {"inverse_diag_panel", &lpgp_ctx::inverse_diag_panel}, {"cv_fold_batch", &lpgp_ctx::cv_fold_batch},
    {"evidence_h2d_bytes", &lpgp_ctx::evidence_h2d_bytes}, {"evidence_d2h_bytes", &lpgp_ctx::evidence_d2h_bytes}};

int lpgp_get_option(lpgp_ctx* ctx, const char* key, int64_t* value) {
  LPGP_CHECK(ctx && key && value, "lpgp_get_option: null argument");
  const int rc = option_get(*ctx, key, value);
  if (rc == 0) return 0;
  if (std::strcmp(key, "live_mats") == 0) {
    *value = ctx->live_mats;
    return 0;
  }
  for (const auto& r : kRoutes)
    if (std::strcmp(key, r.key) == 0) {
      *value = ctx->route.*r.count;
      return 0;
    }
  for (const auto& r : kEvidence)
    if (std::strcmp(key, r.key) == 0) {
      *value = ctx->*r.field;
      return 0;
    }
  return rc;       // (unknown option <key>, set by option_get)
}

int lpgp_set_option(lpgp_ctx* ctx, const char* key, int64_t value) {
  LPGP_DEVICE(ctx);
  if (key && std::strcmp(key, kEvidence[0].key) == 0) {
    LPGP_CHECK(value >= TILE && value <= 4096 && value % TILE == 0, "inverse_diag_panel must be a multiple of %d in %d .. 4096", TILE, TILE);
    ctx->inverse_diag_panel = value;
    return 0;
  }
  if (key && std::strcmp(key, kEvidence[1].key) == 0) {
    LPGP_CHECK(value >= 1 && value <= 65535, "cv_fold_batch must lie in 1 .. 65535 (folds per launch, 256 KiB of scratch each)");
    ctx->cv_fold_batch = value;
    return 0;
  }
  return option_set(*ctx, key, value);
}

// ---- multi-GPU ---------------------------------------------------------------------------
int lpgp_dist_unique_id(char* out128) {
  LPGP_CHECK(out128 != nullptr, "lpgp_dist_unique_id: null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  LPGP_CHECK(r == ncclSuccess, "ncclGetUniqueId: %s", ncclGetErrorString(r));
  std::memcpy(out128, &id, 128);
  return 0;
}

// default process grid for `world` ranks: Pr = world, Pc = 1.  On the full mesh of xGMI links (every GPU a direct
// link to every other) a gathered panel of S bytes costs a link S / Pr: a tall grid keeps
// every link at 1 / world of the panel, shares the panel triangular solve among all ranks and needs no row exchange.
static void choose_grid(lpgp_ctx* ctx, int world) {
  if (ctx->grid_set && ctx->pr * ctx->pc == world) return;
  ctx->pr = world;
  ctx->pc = 1;
}

static int dist_fail(lpgp_ctx* ctx, int rc);

int lpgp_dist_set_grid(lpgp_ctx* ctx, int32_t pr, int32_t pc) {
  LPGP_CHECK(ctx && pr >= 1 && pc >= 1 && pr <= 8 && pc <= 8, "lpgp_dist_set_grid: bad grid %d x %d", pr, pc);
  // before the bring-up, or afterwards while no matrix or right-hand side exists (their storage is laid out for the
  // grid they were created under): bench.py times the same workload on two grids during warm-up and keeps the faster
  if (ctx->distributed()) {
    LPGP_CHECK(pr * pc == ctx->world, "lpgp_dist_set_grid: grid %d x %d does not match %d ranks", pr, pc, ctx->world);
    LPGP_CHECK(ctx->live_mats == 0, "lpgp_dist_set_grid: %d matrices / right-hand sides of the current grid are still alive", ctx->live_mats);
  }
  ctx->pr = pr;
  ctx->pc = pc;
  ctx->grid_set = 1;
  return 0;
}

int lpgp_dist_link_probe(lpgp_ctx* ctx, int64_t bytes, int32_t reps, double* out) {
  LPGP_CHECK(ctx && out && bytes >= 8 && reps >= 1, "lpgp_dist_link_probe: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(ctx->distributed() && !ctx->dist_broken, "lpgp_dist_link_probe: no multi-GPU job (call lpgp_dist_init first)");
  return dist_fail(ctx, dist_link_probe(ctx, bytes, reps, out));
}

int lpgp_dist_grid(lpgp_ctx* ctx, int32_t* pr, int32_t* pc) {
  LPGP_CHECK(ctx != nullptr, "lpgp_dist_grid: null context");
  if (pr) *pr = ctx->pr;
  if (pc) *pc = ctx->pc;
  return 0;
}

int lpgp_dist_stats(lpgp_ctx* ctx, double* bytes_sent, double* bytes_received, int32_t reset) {
  LPGP_CHECK(ctx != nullptr, "lpgp_dist_stats: null context");
  if (bytes_sent) *bytes_sent = ctx->comm_bytes_sent;
  if (bytes_received) *bytes_received = ctx->comm_bytes_recv;
  if (reset) ctx->comm_bytes_sent = ctx->comm_bytes_recv = 0.0;
  return 0;
}

int lpgp_dist_init(lpgp_ctx* ctx, int32_t rank, int32_t world, const char* uid128) {
  LPGP_CHECK(ctx && uid128 && world >= 1 && rank >= 0 && rank < world, "lpgp_dist_init: bad argument");
  LPGP_CHECK(!ctx->distributed(), "lpgp_dist_init: already initialised");
  LPGP_CHECK(!ctx->grid_set || ctx->pr * ctx->pc == world, "lpgp_dist_init: grid %d x %d does not match %d ranks", ctx->pr, ctx->pc, world);
  LPGP_HIP(hipSetDevice(ctx->device));
  ncclUniqueId id;
  std::memcpy(&id, uid128, 128);
  ncclComm_t comm = nullptr;
  ncclResult_t r = ncclCommInitRank(&comm, world, id, rank);
  LPGP_CHECK(r == ncclSuccess, "ncclCommInitRank(rank %d of %d): %s", rank, world, ncclGetErrorString(r));
  ctx->nccl_comm = comm;
  ctx->rank = rank;
  ctx->world = world;
  choose_grid(ctx, world);
  if (world > 1 && ctx->split_gather) {
    // a second communicator for the bulk of split panel gathers (operations on one communicator are serialised: the
    // small exchanges of the panel chain would queue behind it).  Without it the split gather still works, serialised.
    ncclComm_t bulk = nullptr;
    if (ncclCommSplit(comm, 0, rank, &bulk, nullptr) == ncclSuccess) ctx->nccl_comm_bulk = bulk;
  }
  // every connection is made NOW, while all ranks are alive (see dist_warm_up, which also makes the ranks AGREE on the
  // bulk communicator: all of them use it or none does); also the first check that data arrives
  int rc = dist_fail(ctx, dist_warm_up(ctx));
  if (rc != 0) {
    // a failed bring-up leaves a plain single-GPU context behind (the caller may try another transport, or run replicas)
    ctx->rank = 0;
    ctx->world = 1;
    if (!ctx->grid_set) ctx->pr = ctx->pc = 1;
    ctx->dist_broken = 0;
  }
  return rc;
}

int lpgp_dist_init_host(lpgp_ctx* ctx, int32_t rank, int32_t world, lpgp_host_exchange_fn fn, void* user) {
  LPGP_CHECK(ctx && fn && world >= 1 && rank >= 0 && rank < world, "lpgp_dist_init_host: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "lpgp_dist_init_host: already initialised");
  LPGP_CHECK(!ctx->grid_set || ctx->pr * ctx->pc == world, "lpgp_dist_init_host: grid %d x %d does not match %d ranks", ctx->pr, ctx->pc, world);
  ctx->host_xfer = fn;
  ctx->host_xfer_user = user;
  ctx->rank = rank;
  ctx->world = world;
  choose_grid(ctx, world);
  return 0;
}

int lpgp_dist_ipc_export(lpgp_ctx* ctx, int64_t window_bytes, char* handle64) {
  LPGP_CHECK(ctx && handle64 && window_bytes >= (int64_t)(1 << 20), "lpgp_dist_ipc_export: bad argument (window of at least 1 MiB)");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed() && !ctx->ipc_window, "lpgp_dist_ipc_export: already initialised");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t size");
  const size_t doubles = (size_t)window_bytes / sizeof(double);
  LPGP_HIP(hipMalloc(&ctx->ipc_window, doubles * sizeof(double)));
  ctx->ipc_window_doubles = doubles;
  hipIpcMemHandle_t h;
  LPGP_HIP(hipIpcGetMemHandle(&h, ctx->ipc_window));
  std::memcpy(handle64, &h, 64);
  return 0;
}

int lpgp_dist_init_ipc(lpgp_ctx* ctx, int32_t rank, int32_t world, const char* handles, lpgp_host_exchange_fn fn, void* user) {
  LPGP_CHECK(ctx && handles && fn && world >= 1 && rank >= 0 && rank < world, "lpgp_dist_init_ipc: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed() && ctx->ipc_window, "lpgp_dist_init_ipc: call lpgp_dist_ipc_export first (once)");
  LPGP_CHECK(!ctx->grid_set || ctx->pr * ctx->pc == world, "lpgp_dist_init_ipc: grid %d x %d does not match %d ranks", ctx->pr, ctx->pc, world);
  ctx->ipc_peer.assign((size_t)world, nullptr);
  for (int r = 0; r < world; ++r) {
    if (r == rank) {
      ctx->ipc_peer[r] = ctx->ipc_window;
      continue;
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, handles + (size_t)r * 64, 64);
    void* p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      set_error("lpgp_dist_init_ipc: hipIpcOpenMemHandle for the window of rank %d: %s", r, hipGetErrorString(e));
      ctx->ipc_peer.clear();
      return -1;
    }
    ctx->ipc_peer[r] = (double*)p;
  }
  ctx->host_xfer = fn;                 // barriers and the info all-reduce travel over the caller's control plane
  ctx->host_xfer_user = user;
  ctx->rank = rank;
  ctx->world = world;
  choose_grid(ctx, world);
  return 0;
}

int lpgp_dist_info(lpgp_ctx* ctx, int32_t* rank, int32_t* world) {
  LPGP_DEVICE(ctx);
  if (rank) *rank = ctx->rank;
  if (world) *world = ctx->world;
  return 0;
}

// ---- points ----------------------------------------------------------------------------
int lpgp_pts_create(lpgp_ctx* ctx, const double* X_host, int64_t n, int32_t d, lpgp_pts** out) {
  LPGP_CHECK(ctx && X_host && out, "lpgp_pts_create: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(n >= 0 && d >= 1 && d <= LPGP_MAXD, "lpgp_pts_create: n=%lld d=%d", (long long)n, d);
  std::unique_ptr<lpgp_pts> p(new lpgp_pts());
  p->ctx = ctx;
  p->n = n;
  p->d = d;
  p->n_pad = round_up(n > 0 ? n : 1, 64);
  const size_t bytes = (size_t)p->n_pad * d * sizeof(double);
  const bool recycle = !ctx->distributed() && !ctx->single_stream;
  // the buffer: a recycled one of about the size (lpgp_internal.h: pts_pool), else a new one
  DevBuf x;
  if (recycle) {
    int best = -1;
    for (int i = 0; i < (int)ctx->pts_pool.size(); ++i) {
      const auto& b = ctx->pts_pool[i];
      if (b.bytes >= bytes && b.bytes <= 2 * bytes + 4096 && (best < 0 || b.bytes < ctx->pts_pool[best].bytes)) best = i;
    }
    if (best >= 0) {
      x.adopt_raw(ctx->pts_pool[best].p);
      p->bytes = ctx->pts_pool[best].bytes;
      ctx->pts_pool.erase(ctx->pts_pool.begin() + best);
    }
  }
  if (!x.as()) {
    LPGP_TRY(DevBuf::raw(bytes, &x));
    p->bytes = bytes;
  }
  auto fill = [&](double* soa) {
    std::memset(soa, 0, bytes);
    for (int64_t i = 0; i < n; ++i)
      for (int j = 0; j < d; ++j) soa[(size_t)j * p->n_pad + i] = X_host[i * d + j];
  };
  if (recycle && bytes <= lpgp_ctx::PTS_SLOT_BYTES) {
    // small: through the next pinned slot, on the panel stream, no wait (the slot is reused after its copy has completed)
    lpgp_ctx::PtsSlot& sl = ctx->pts_ring[ctx->pts_next];
    ctx->pts_next = (ctx->pts_next + 1) % lpgp_ctx::PTS_SLOTS;
    if (!sl.h) {
      LPGP_HIP(hipHostMalloc(&sl.h, lpgp_ctx::PTS_SLOT_BYTES, hipHostMallocDefault));
      LPGP_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    } else if (sl.used) {
      LPGP_HIP(hipEventSynchronize(sl.done));
    }
    fill((double*)sl.h);
    LPGP_HIP(hipMemcpyAsync(x.as(), sl.h, bytes, hipMemcpyHostToDevice, ctx->s_main));
    LPGP_HIP(hipEventRecord(sl.done, ctx->s_main));
    sl.used = true;
  } else {
    std::vector<double> soa((size_t)p->n_pad * d);
    fill(soa.data());
    StreamDrain drain{ctx->s_main};
    // (a recycled buffer may still be read by kernels on the panel stream: the copy is ordered behind them there)
    LPGP_HIP(hipMemcpyAsync(x.as(), soa.data(), bytes, hipMemcpyHostToDevice, ctx->s_main));
    LPGP_TRY(drain.wait());
  }
  p->x = (double*)x.release();
  *out = p.release();
  return 0;
}

int lpgp_pts_destroy(lpgp_pts* p) {
  if (!p) return 0;
  lpgp_ctx* ctx = p->ctx;
  (void)hipSetDevice(ctx->device);
  // recycled: whatever still reads it runs on the panel stream, where the next owner's upload is ordered behind it
  if (!ctx->distributed() && !ctx->single_stream && ctx->pts_pool.size() < 32 && p->bytes <= ((size_t)4 << 20))
    ctx->pts_pool.push_back({p->x, p->bytes});
  else
    (void)hipFree(p->x);
  delete p;
  return 0;
}

// ---- matrix ----------------------------------------------------------------------------
int lpgp_mat_create(lpgp_ctx* ctx, int64_t capacity_hint, lpgp_mat** out) {
  LPGP_CHECK(ctx && out, "lpgp_mat_create: null argument");
  LPGP_DEVICE(ctx);
  std::unique_ptr<lpgp_mat> m(new lpgp_mat());
  m->ctx = ctx;
  int64_t cap = round_up(capacity_hint > 0 ? capacity_hint : 8 * TILE, TILE);      // (no hint: room for 1 024 rows, 8 MB -- the reference's own problem sizes start here)
  LPGP_TRY(mat_alloc(ctx, m.get(), cap));
  ++ctx->live_mats;
  *out = m.release();
  return 0;
}

int lpgp_mat_destroy(lpgp_mat* m) {
  if (!m) return 0;
  (void)hipSetDevice(m->ctx->device);
  mat_release(m->ctx, m);
  --m->ctx->live_mats;
  delete m;
  return 0;
}

static int mat_add_block_impl(lpgp_ctx* ctx, lpgp_mat* mat, int64_t n, bool pad_now);
int lpgp_mat_add_block(lpgp_ctx* ctx, lpgp_mat* mat, int64_t n) { return mat_add_block_impl(ctx, mat, n, true); }
// pad_now = false: the caller launches the identity tail itself (lpgp_mat_condition: together with the noise, launch_finish_block)
static int mat_add_block_impl(lpgp_ctx* ctx, lpgp_mat* mat, int64_t n, bool pad_now) {
  LPGP_CHECK(ctx && mat && n > 0, "lpgp_mat_add_block: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_mat_add_block");
  LPGP_CHECK(mat->hidden.empty(), "lpgp_mat_add_block: a strict prefix of the blocks is in view (lpgp_mat_set_view); extend a clone instead");
  const lpgp_block b = mat->next_block(n);
  if (b.poff + b.pn > mat->cap) {
    // grow geometrically while the matrix is small (a chain of small conditionings without `gram_capacity_hint` used to
    // re-allocate, copy and synchronise at EVERY block: 48 us of host time per add_block at N_tot = 1 152); a block that
    // needs more than that gets exactly what it needs (the large PDE block of c3 / c4 is the last growth of its chain)
    int64_t want = b.poff + b.pn;
    const int64_t geo = round_up(mat->cap + mat->cap / 2, TILE);
    // ... capped by BYTES, not rows (a chain that needed just over 10 923 rows got a 16 384^2 matrix, 2.1 GB and
    // a full copy, about twice what it asked for): at most 256 MB of storage beyond the request
    if (geo > want && (geo * geo - want * want) * (int64_t)sizeof(double) <= ((int64_t)256 << 20)) want = geo;
    int rc = mat_alloc(ctx, mat, want);
    if (rc != 0) return rc;
  }
  const int64_t pad = b.pn - b.n;
  if (pad > 0 && pad_now) {
    // identity tail of the block: zero the pad rows (all columns up to the block end) and the
    // pad columns (all rows down to the capacity), then ones on the diagonal
    const Layout2D lay = mat_layout(ctx);
    const int64_t r0 = b.poff + b.n;
    launch_pad_block(ctx->s_main, mat->a, mat->lr_cap, r0, pad, mat->cap, lay);
    LPGP_HIP(hipGetLastError());
  }
  return mat->push_block(n);
}

int lpgp_mat_pop_block(lpgp_ctx* ctx, lpgp_mat* mat) {
  LPGP_CHECK(ctx && mat, "lpgp_mat_pop_block: null argument");
  LPGP_DEVICE(ctx);
  std::string err;
  LPGP_TRY(refused(mat->can_pop_block(&err), err));
  LPGP_TRY(sync_stream(ctx, ctx->s_main));          // nothing of a failed append still in flight (watched: an exchange with a dead peer may be pending)
  return refused(mat->pop_block(&err), err);
}

int32_t lpgp_mat_num_blocks(const lpgp_mat* mat) { return mat ? (int32_t)mat->blocks.size() : -1; }
int32_t lpgp_mat_num_blocks_total(const lpgp_mat* mat) { return mat ? (int32_t)mat->total_blocks() : -1; }

int lpgp_mat_set_view(lpgp_ctx* ctx, lpgp_mat* mat, int32_t nblocks) {
  LPGP_CHECK(ctx && mat, "lpgp_mat_set_view: null argument");
  std::string err;
  return refused(mat->set_view(nblocks, &err), err);
}

// deleter of a handle that is still under construction but already owns device memory and is counted in live_mats
struct LPGP_LOCAL Destroy {
  void operator()(lpgp_mat* m) const { (void)lpgp_mat_destroy(m); }
  void operator()(lpgp_rhs* r) const { (void)lpgp_rhs_destroy(r); }
};

int lpgp_mat_clone(lpgp_ctx* ctx, const lpgp_mat* src, int32_t nblocks, lpgp_mat** out) {
  LPGP_CHECK(ctx && src && out, "lpgp_mat_clone: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(src, "lpgp_mat_clone");
  LPGP_CHECK(!ctx->distributed(), "lpgp_mat_clone: not available in a multi-GPU job");
  std::string err;
  LPGP_TRY(refused(src->can_take_prefix("lpgp_mat_clone", nblocks, false, &err), err));
  const int64_t pn = src->padded_end(nblocks);
  lpgp_mat* created = nullptr;
  LPGP_TRY(lpgp_mat_create(ctx, pn, &created));
  std::unique_ptr<lpgp_mat, Destroy> m(created);
  LPGP_HIP(hipMemcpy2DAsync(m->a, (size_t)m->lr_cap * sizeof(double), src->a, (size_t)src->lr_cap * sizeof(double),
                            (size_t)pn * sizeof(double), (size_t)pn, hipMemcpyDeviceToDevice, ctx->s_main));
  LPGP_HIP(hipMemcpyAsync(m->linv, src->linv, (size_t)pn * TILE * sizeof(double), hipMemcpyDeviceToDevice, ctx->s_main));
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));
  LPGP_TRY(refused(m->adopt_prefix(*src, nblocks, &err), err));
  *out = m.release();
  return 0;
}

int64_t lpgp_mat_size(const lpgp_mat* mat) { return mat ? mat->n : -1; }
int64_t lpgp_mat_padded_size(const lpgp_mat* mat) { return mat ? mat->pn : -1; }

// What the lpgp_gram_assemble* entry points ask of their target: block (bi, bj) of the lower triangle, not factored yet, and the
// second point set (`second`: X1 / F1) NULL exactly on the diagonal.
static int gram_target(const char* fn, const lpgp_mat* mat, int32_t bi, int32_t bj, const void* second, const char* second_name) {
  LPGP_CHECK(bi >= 0 && bi < (int)mat->blocks.size() && bj >= 0 && bj <= bi, "%s: bad block (%d,%d)", fn, bi, bj);
  LPGP_CHECK(mat->blocks[bi].poff >= mat->pn_fact, "%s: block %d is already factored", fn, bi);
  LPGP_CHECK((second == nullptr) == (bi == bj), "%s: %s must be NULL exactly for diagonal blocks", fn, second_name);
  return 0;
}

int lpgp_gram_assemble(lpgp_ctx* ctx, const lpgp_kdesc* kd, int32_t ngroups, const lpgp_pts* X0,
                       const lpgp_pts* X1, lpgp_mat* mat, int32_t bi, int32_t bj) {
  LPGP_CHECK(ctx && kd && X0 && mat, "lpgp_gram_assemble: null argument");
  LPGP_DEVICE(ctx);
  LPGP_TRY(gram_target("lpgp_gram_assemble", mat, bi, bj, X1, "X1"));
  const lpgp_block& Bi = mat->blocks[bi];
  const lpgp_block& Bj = mat->blocks[bj];
  LPGP_CHECK(X0->n == Bi.n, "lpgp_gram_assemble: X0 has %lld points, block %d has %lld rows", (long long)X0->n, bi, (long long)Bi.n);
  const bool sym = (bi == bj);
  const lpgp_pts* Xc = sym ? X0 : X1;
  LPGP_CHECK(Xc->n == Bj.n && Xc->d == X0->d && kd[0].d == X0->d, "lpgp_gram_assemble: shape mismatch");
  DevDesc desc;
  int rc = lower_kdesc(kd, ngroups, &desc);
  if (rc != 0) return rc;
  // distributed factorisation: a rank assembles only the columns of the panels it will factor
  // (the others arrive as factored panels); columns that are already factored (cross blocks of
  // a block append) are needed by every rank
  // multi-GPU: a rank evaluates exactly the tiles it owns (2-D block-cyclic), zero communication
  rc = launch_assemble(ctx, ctx->s_main, desc, X0->x, X0->n, X0->n_pad, Xc->x, Xc->n, Xc->n_pad, mat->a, mat->lr_cap,
                       Bi.poff, Bj.poff, sym ? 1 : 0, mat_layout(ctx));
  return rc;       // asynchronous: consumers are ordered behind it on the main stream
}

int lpgp_gram_assemble_weighted(lpgp_ctx* ctx, const lpgp_wpair* pairs, int32_t npairs, const double* w0_host, int32_t A0,
                                const double* w1_host, int32_t A1, const lpgp_pts* X0, const lpgp_pts* X1, lpgp_mat* mat, int32_t bi,
                                int32_t bj) {
  static const char* fn = "lpgp_gram_assemble_weighted";
  LPGP_CHECK(ctx && X0 && mat, "%s: null argument", fn);
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "%s: single GPU only (this context has joined a multi-GPU job)", fn);
  LPGP_MAT_ALIVE(mat, "lpgp_gram_assemble_weighted");
  LPGP_CHECK(mat->hidden.empty(), "%s: a strict prefix of the blocks is in view (lpgp_mat_set_view)", fn);
  LPGP_TRY(gram_target(fn, mat, bi, bj, X1, "X1"));
  const lpgp_block& Bi = mat->blocks[bi];
  const lpgp_block& Bj = mat->blocks[bj];
  const bool sym = (bi == bj);
  LPGP_CHECK(w0_host != nullptr, "%s: null row weights", fn);
  LPGP_CHECK(sym ? w1_host == nullptr : w1_host != nullptr, "%s: the column weights must be NULL exactly for diagonal blocks", fn);
  LPGP_TRY_RC(check_wpairs(pairs, npairs, A0, A1, sym ? WP_SYM : WP_RECT, fn));
  const lpgp_pts* Xc = sym ? X0 : X1;
  LPGP_CHECK(X0->n == Bi.n && Xc->n == Bj.n && Xc->d == X0->d && pairs[0].kd[0].d == X0->d, "%s: shape mismatch", fn);
  return assemble_weighted(ctx, ctx->s_main, pairs, npairs, w0_host, A0, w1_host, sym ? A0 : A1, X0, Xc, sym, mat->a, mat->lr_cap, Bi.poff,
                           Bj.poff, mat_layout(ctx));
}

// ---- observations through a matrix: stencil tables (mix_table.h) and their assembly (assemble_mixed_kernel) --------------------
int lpgp_mix_create(lpgp_ctx* ctx, int64_t q, int32_t S, const int32_t* idx_host, const double* w_host, int64_t npts, lpgp_mix** out) {
  static_assert(MIX_MAXS == LPGP_MAXS, "the row width of a stencil table");
  LPGP_CHECK(ctx && out, "lpgp_mix_create: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "lpgp_mix_create: single GPU only (this context has joined a multi-GPU job)");
  MixTable t;
  std::string err;
  LPGP_TRY(refused(mix_table_build(q, S, idx_host, w_host, npts, &t, &err), "lpgp_mix_create: " + err));
  const size_t w_bytes = t.w.size() * sizeof(double), idx_bytes = t.idx.size() * sizeof(int32_t);
  DevBuf buf;
  LPGP_TRY(DevBuf::raw(w_bytes + idx_bytes, &buf));
  {
    StreamDrain drain{ctx->s_main};                 // (behind `t` and `buf`: the copies out of `t` have landed before either goes)
    LPGP_HIP(hipMemcpyAsync(buf.as<char>(), t.w.data(), w_bytes, hipMemcpyHostToDevice, ctx->s_main));
    LPGP_HIP(hipMemcpyAsync(buf.as<char>() + w_bytes, t.idx.data(), idx_bytes, hipMemcpyHostToDevice, ctx->s_main));
    LPGP_TRY(drain.wait());
  }
  std::unique_ptr<lpgp_mix> m(new lpgp_mix());
  m->ctx = ctx;
  m->q = t.q;
  m->S = t.S;
  m->npts = t.npts;
  m->w = (double*)buf.release();
  m->idx = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(m->w) + w_bytes);
  *out = m.release();
  return 0;
}

int lpgp_mix_destroy(lpgp_mix* m) {
  if (!m) return 0;
  (void)hipSetDevice(m->ctx->device);
  (void)hipFree(m->w);                              // (waits for the device: no kernel still reads the table)
  delete m;
  return 0;
}

// what the mixed assemblies ask of one side: points of this context, and a table (if any) of this context, made for these points
static int mix_side(const char* fn, const lpgp_ctx* ctx, const lpgp_pts* X, const lpgp_mix* M, const char* side, int64_t* rows) {
  LPGP_CHECK(X->ctx == ctx, "%s: the %s points belong to another context", fn, side);
  if (M) {
    LPGP_CHECK(M->ctx == ctx, "%s: the %s stencil table belongs to another context", fn, side);
    LPGP_CHECK(M->npts == X->n, "%s: the %s stencil table was made for %lld points, the point set has %lld", fn, side, (long long)M->npts,
               (long long)X->n);
  }
  *rows = M ? M->q : X->n;
  return 0;
}

int lpgp_gram_assemble_mixed(lpgp_ctx* ctx, const lpgp_kdesc* kd, int32_t ngroups, const lpgp_pts* X0, const lpgp_mix* M0, const lpgp_pts* X1,
                             const lpgp_mix* M1, lpgp_mat* mat, int32_t bi, int32_t bj) {
  static const char* fn = "lpgp_gram_assemble_mixed";
  LPGP_CHECK(ctx && kd && X0 && mat, "%s: null argument", fn);
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "%s: single GPU only (this context has joined a multi-GPU job)", fn);
  LPGP_CHECK(mat->ctx == ctx, "%s: the matrix belongs to another context", fn);
  LPGP_MAT_ALIVE(mat, "lpgp_gram_assemble_mixed");
  LPGP_CHECK(mat->hidden.empty(), "%s: a strict prefix of the blocks is in view (lpgp_mat_set_view)", fn);
  LPGP_TRY(gram_target(fn, mat, bi, bj, X1, "X1"));
  const bool sym = (bi == bj);
  LPGP_CHECK(!sym || M1 == nullptr, "%s: M1 must be NULL for a diagonal block (M0 serves both sides)", fn);
  const lpgp_pts* Xc = sym ? X0 : X1;
  const lpgp_mix* Mc = sym ? M0 : M1;
  int64_t rows = 0, cols = 0;
  LPGP_TRY(mix_side(fn, ctx, X0, M0, "row", &rows));
  LPGP_TRY(mix_side(fn, ctx, Xc, Mc, "column", &cols));
  const lpgp_block& Bi = mat->blocks[bi];
  const lpgp_block& Bj = mat->blocks[bj];
  LPGP_CHECK(rows == Bi.n, "%s: the row side has %lld rows, block %d has %lld", fn, (long long)rows, bi, (long long)Bi.n);
  LPGP_CHECK(cols == Bj.n, "%s: the column side has %lld rows, block %d has %lld", fn, (long long)cols, bj, (long long)Bj.n);
  LPGP_CHECK(Xc->d == X0->d && kd[0].d == X0->d, "%s: dimension mismatch: the descriptor has d=%d, the points d=%d and d=%d", fn, kd[0].d, X0->d, Xc->d);
  DevDesc desc;
  LPGP_TRY(lower_kdesc(kd, ngroups, &desc));
  return assemble_mixed(ctx, ctx->s_main, desc, X0, M0, Xc, Mc, sym, mat->a, mat->lr_cap, Bi.poff, Bj.poff, mat_layout(ctx));
}

int lpgp_kron_fits(const lpgp_kdesc* kd, int32_t ngroups) { return kron_fits(kd, ngroups) ? 1 : 0; }

int lpgp_gram_assemble_grid(lpgp_ctx* ctx, const lpgp_kdesc* kd, int32_t ngroups, const lpgp_pts* const* F0,
                            const lpgp_pts* const* F1, lpgp_mat* mat, int32_t bi, int32_t bj) {
  LPGP_CHECK(ctx && kd && F0 && mat, "lpgp_gram_assemble_grid: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(ngroups >= 1 && ngroups <= LPGP_MAXG, "lpgp_gram_assemble_grid: bad ngroups %d", ngroups);
  LPGP_TRY(gram_target("lpgp_gram_assemble_grid", mat, bi, bj, F1, "F1"));
  const lpgp_block& Bi = mat->blocks[bi];
  const lpgp_block& Bj = mat->blocks[bj];
  const bool sym = (bi == bj);
  const int D = kd[0].d;
  LPGP_CHECK(D >= 1 && D <= LPGP_MAXD, "lpgp_gram_assemble_grid: d=%d", D);
  LPGP_CHECK(kron_fits(kd, ngroups), "lpgp_gram_assemble_grid: the Kronecker path does not hold this sum (lpgp_kron_fits tells beforehand)");
  const double *f0[LPGP_MAXD], *f1[LPGP_MAXD];
  int64_t n0d[LPGP_MAXD], n1d[LPGP_MAXD], n0 = 1, n1 = 1;
  for (int d = 0; d < D; ++d) {
    const lpgp_pts* a = F0[d];
    const lpgp_pts* b = sym ? F0[d] : F1[d];
    LPGP_CHECK(a && b && a->d == 1 && b->d == 1 && a->n >= 1 && b->n >= 1, "lpgp_gram_assemble_grid: factor %d must be a 1-D point set", d);
    f0[d] = a->x; f1[d] = b->x;
    n0d[d] = a->n; n1d[d] = b->n;
    n0 *= a->n; n1 *= b->n;
  }
  LPGP_CHECK(n0 == Bi.n && n1 == Bj.n, "lpgp_gram_assemble_grid: grids have %lld x %lld points, block (%d,%d) is %lld x %lld",
             (long long)n0, (long long)n1, bi, bj, (long long)Bi.n, (long long)Bj.n);
  const size_t wd = kron_work_doubles(D, n0d, n1d);
  DevBuf work;                                     // (reuse is ordered behind the launch on the main stream)
  LPGP_TRY(DevBuf::pool(ctx, wd * sizeof(double), &work));
  return launch_assemble_kron(ctx, ctx->s_main, kd, ngroups, f0, n0d, f1, n1d, work.as(), wd, mat->a, mat->lr_cap,
                              Bi.poff, Bj.poff, sym ? 1 : 0, mat_layout(ctx));
}

int lpgp_mat_add_diag(lpgp_ctx* ctx, lpgp_mat* mat, int32_t bi, const double* v_host, double scalar) {
  LPGP_CHECK(ctx && mat && bi >= 0 && bi < (int)mat->blocks.size(), "lpgp_mat_add_diag: bad argument");
  LPGP_DEVICE(ctx);
  const lpgp_block& B = mat->blocks[bi];
  LPGP_CHECK(B.poff >= mat->pn_fact, "lpgp_mat_add_diag: block %d is already factored", bi);
  double* dv = nullptr;
  if (v_host) {
    int rc = ensure_tmp(ctx, B.n);
    if (rc != 0) return rc;
    LPGP_HIP(hipMemcpyAsync(ctx->d_tmp, v_host, (size_t)B.n * sizeof(double), hipMemcpyHostToDevice, ctx->s_main));
    dv = ctx->d_tmp;
  }
  int rc = launch_add_diag(ctx->s_main, mat->a, mat->lr_cap, B.poff, B.n, dv, scalar, mat_layout(ctx));
  if (rc != 0) return rc;
  if (v_host) LPGP_HIP(hipStreamSynchronize(ctx->s_main));     // borrowed host vector, shared scratch
  return 0;
}

int lpgp_mat_add_dense(lpgp_ctx* ctx, lpgp_mat* mat, int32_t bi, const double* B_host) {
  LPGP_CHECK(ctx && mat && B_host && bi >= 0 && bi < (int)mat->blocks.size(), "lpgp_mat_add_dense: bad argument");
  LPGP_DEVICE(ctx);
  const lpgp_block& B = mat->blocks[bi];
  LPGP_CHECK(B.poff >= mat->pn_fact, "lpgp_mat_add_dense: block %d is already factored", bi);
  int rc = ensure_tmp(ctx, B.n * B.n);
  if (rc != 0) return rc;
  LPGP_HIP(hipMemcpyAsync(ctx->d_tmp, B_host, (size_t)(B.n * B.n) * sizeof(double), hipMemcpyHostToDevice, ctx->s_main));
  rc = launch_add_dense(ctx->s_main, mat->a, mat->lr_cap, B.poff, B.n, ctx->d_tmp, mat_layout(ctx));
  if (rc != 0) return rc;
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));
  return 0;
}

// A failure inside a collective call on ONE rank (HIP error, failed allocation, RCCL error) would leave the other
// ranks blocked in their next send / receive for ever: abort the communicator, which makes every pending and later
// RCCL call on every rank of the job return an error instead.  The context is unusable afterwards.
static int dist_fail(lpgp_ctx* ctx, int rc) {
  if (rc != 0 && ctx->nccl_comm && ctx->world > 1) {
    (void)ncclCommAbort((ncclComm_t)ctx->nccl_comm);
    if (ctx->nccl_comm_bulk) (void)ncclCommAbort((ncclComm_t)ctx->nccl_comm_bulk);
    ctx->nccl_comm = ctx->nccl_comm_bulk = nullptr;
    ctx->dist_broken = 1;
  }
  return rc;
}

// V <- L^{-1} V and V <- L^{-T} V for the whole view of `mat`: streamed over the ranks of a multi-GPU job (a failure of one
// rank aborts the communicator), blocked on a single GPU
static int solve_lower(lpgp_ctx* ctx, lpgp_mat* mat, double* v, int64_t ldv, int64_t m_pad) {
  if (ctx->distributed()) return dist_fail(ctx, trsm_lower_dist(ctx, mat, mat->pn / TILE, v, ldv, m_pad));
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  return trsm_lower_blocked(ctx, F, mat->pn / TILE, v, ldv, m_pad);
}
static int solve_lower_t(lpgp_ctx* ctx, lpgp_mat* mat, double* v, int64_t ldv, int64_t m_pad) {
  if (ctx->distributed()) return dist_fail(ctx, trsm_lower_t_dist(ctx, mat, mat->pn / TILE, v, ldv, m_pad));
  FactorView F;
  LPGP_TRY(factor_view(mat, &F));
  return trsm_lower_t_blocked(ctx, F, mat->pn / TILE, v, ldv, m_pad);
}

int lpgp_mat_to_host(lpgp_ctx* ctx, lpgp_mat* mat, int32_t what, double* out_host) {
  LPGP_CHECK(ctx && mat && out_host, "lpgp_mat_to_host: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_mat_to_host");
  LPGP_CHECK(what == 0 || what == 1, "lpgp_mat_to_host: what must be 0 or 1");
  if (what == 0) LPGP_CHECK(mat->pn_fact == 0, "lpgp_mat_to_host: Gram no longer available after potrf");
  if (what == 1) LPGP_CHECK(mat->pn_fact == mat->pn, "lpgp_mat_to_host: matrix is not (fully) factored");
  const int64_t pn = mat->pn, n = mat->n;
  std::vector<double> tmp((size_t)pn * pn);
  LPGP_TRY(sync_stream(ctx, ctx->s_main));           // assembly launches are asynchronous
  if (ctx->distributed()) {
    LPGP_CHECK(what == 1, "lpgp_mat_to_host: only the factor can be collected in a multi-GPU job");
    int rc = dist_fail(ctx, factor_to_host_dist(ctx, mat, tmp.data()));      // collective: the factor is streamed to every rank
    if (rc != 0) return rc;
  } else
  LPGP_HIP(hipMemcpy2D(tmp.data(), (size_t)pn * sizeof(double), mat->a, (size_t)mat->lr_cap * sizeof(double),
                       (size_t)pn * sizeof(double), (size_t)pn, hipMemcpyDeviceToHost));
  // tmp is column-major pn x pn: element (r,c) at tmp[r + c*pn]
  for (const auto& bi : mat->blocks)
    for (const auto& bj : mat->blocks)
      for (int64_t i = 0; i < bi.n; ++i)
        for (int64_t j = 0; j < bj.n; ++j) {
          const int64_t r = bi.poff + i, c = bj.poff + j;
          double v;
          if (r >= c) v = tmp[(size_t)(r + c * pn)];
          else v = (what == 0) ? tmp[(size_t)(c + r * pn)] : 0.0;
          out_host[(bi.off + i) * n + (bj.off + j)] = v;
        }
  return 0;
}

int lpgp_mat_factor_diag(lpgp_ctx* ctx, lpgp_mat* mat, double* out_host) {
  LPGP_CHECK(ctx && mat && out_host, "lpgp_mat_factor_diag: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_mat_factor_diag");
  LPGP_CHECK(mat->pn_fact == mat->pn, "lpgp_mat_factor_diag: matrix is not (fully) factored");
  const int64_t pn = mat->pn;
  if (pn == 0) return 0;
  std::vector<double> tmp((size_t)pn);
  LPGP_TRY(sync_stream(ctx, ctx->s_main));
  if (ctx->distributed()) {
    // replicated diagonal blocks: block K at dblk + K nb^2, leading dimension nb
    const int64_t nb = ctx->nb;
    for (int64_t k0 = 0; k0 < pn; k0 += nb) {
      const int64_t h = std::min(nb, pn - k0);
      LPGP_HIP(hipMemcpy2D(tmp.data() + k0, sizeof(double), mat->dblk + (k0 / nb) * nb * nb, (size_t)(nb + 1) * sizeof(double),
                           sizeof(double), (size_t)h, hipMemcpyDeviceToHost));
    }
  } else {
    LPGP_HIP(hipMemcpy2D(tmp.data(), sizeof(double), mat->a, (size_t)(mat->lr_cap + 1) * sizeof(double), sizeof(double), (size_t)pn,
                         hipMemcpyDeviceToHost));
  }
  mat->gather_padded(tmp.data(), out_host);
  return 0;
}

// ---- factor + solve -----------------------------------------------------------------------
// lpgp_potrf, in the form `form` (TileForm::newton: lpgp_mat_cv's large folds, single GPU; such a factorisation runs without the resident chain)
extern "C++" int lpgp::potrf_mat(lpgp_ctx* ctx, lpgp_mat* mat, int32_t* info, TileForm form) {
  LPGP_CHECK(ctx && mat, "lpgp_potrf: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_potrf");
  if (info) *info = 0;
  if (mat->pn_fact == mat->pn) return 0;
  LPGP_CHECK(mat->hidden.empty(), "lpgp_potrf: a strict prefix of the blocks is in view");
  int32_t h = 0;
  LPGP_CHECK(!ctx->dist_broken, "lpgp_potrf: the communicator was aborted after an earlier failure");
  LPGP_CHECK(form == TileForm::plain || !ctx->distributed(), "lpgp_potrf: the multi-GPU factorisation has the plain tile form only");
  int rc = ctx->distributed()
               ? dist_fail(ctx, potrf_dist(ctx, mat, mat->pn_fact / TILE, mat->pn / TILE, &h))
               : potrf_blocked(ctx, mat, mat->pn_fact / TILE, mat->pn / TILE, &h, form);
  if (rc != 0) {
    mat->poison();                   // (the matrix is partly overwritten in place, pn_fact unchanged: not a state to factor again from)
    return rc;
  }
  if (info) *info = h;
  mat->factored(h);
  return 0;
}

int lpgp_potrf(lpgp_ctx* ctx, lpgp_mat* mat, int32_t* info) { return potrf_mat(ctx, mat, info, TileForm::plain); }

int lpgp_potrf_enqueue(lpgp_ctx* ctx, lpgp_mat* mat) {
  LPGP_CHECK(ctx && mat, "lpgp_potrf_enqueue: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_potrf_enqueue");
  if (mat->pn_fact == mat->pn) return 0;
  LPGP_CHECK(mat->hidden.empty(), "lpgp_potrf_enqueue: a strict prefix of the blocks is in view");
  LPGP_CHECK(!ctx->distributed(), "lpgp_potrf_enqueue: single GPU only (the multi-GPU factorisation agrees on its status collectively: lpgp_potrf)");
  int rc = potrf_blocked(ctx, mat, mat->pn_fact / TILE, mat->pn / TILE, nullptr);
  if (rc != 0) {
    mat->poison();
    return rc;
  }
  mat->factor_enqueued(false);     // (provisionally: lpgp_mat_check / lpgp_mat_truncate take it back on failure)
  return 0;
}

// Consecutive entries of a block row that share a descriptor (value observations against value observations: the whole row incl.
// the diagonal block; the cross blocks of a differential block against the boundary blocks; the rows of a cross-covariance) go
// into as few launches as the job table allows (assemble.hip: launch_assemble_batch).  Owns the descriptor and the jobs of the
// pending run; add() launches it first when the descriptor changes, flush() launches what is pending.
struct LPGP_LOCAL AsmRun {
  lpgp_ctx* ctx;
  double* out;                     // where the blocks go: column-major with leading dimension ld, laid out by lay
  int64_t ld;
  Layout2D lay;
  std::vector<char>* assembled = nullptr;      // rows of a cross-covariance: entry `block` is set once that block's launch is issued
  DevDesc desc;
  std::vector<AsmJob> jobs;
  std::vector<int> blocks;
  int add(const DevDesc& d, const AsmJob& job, int block = -1) {
    if (!jobs.empty() && !assemble_same_fast(desc, d)) LPGP_TRY(flush());
    if (jobs.empty()) desc = d;
    jobs.push_back(job);
    blocks.push_back(block);
    return 0;
  }
  int flush() {
    if (jobs.empty()) return 0;
    const int rc = launch_assemble_batch(ctx, ctx->s_main, desc, jobs.data(), (int)jobs.size(), out, ld, lay);
    if (rc == 0 && assembled)
      for (int b : blocks)
        if (b >= 0 && b < (int)assembled->size()) (*assembled)[(size_t)b] = 1;
    jobs.clear();
    blocks.clear();
    return rc;
  }
};

// The block a conditioning has declared is dropped again on every way out but the good one; the error text of the step that
// failed stays (lpgp_mat_pop_block succeeds and would not touch it, but be explicit).
struct LPGP_LOCAL PopBlock {
  lpgp_ctx* ctx;
  lpgp_mat* mat;
  bool armed = true;
  ~PopBlock() {
    if (!armed) return;
    const std::string msg = lpgp::last_error();
    (void)lpgp_mat_pop_block(ctx, mat);
    set_error("%s", msg.c_str());
  }
};

// identity tail of block B and its noise (dn entries: dv[i] + dscalar) in ONE launch behind the assembly (launch_finish_block)
static int finish_block(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_block& B, int64_t dn, const double* dv, double dscalar) {
  launch_finish_block(ctx->s_main, mat->a, mat->lr_cap, B.poff + B.n, B.pn - B.n, mat->cap, mat_layout(ctx), B.poff, dn, dv, dscalar);
  const hipError_t e = hipGetLastError();
  LPGP_CHECK(e == hipSuccess, "lpgp_mat_condition: %s", hipGetErrorString(e));
  return 0;
}

int lpgp_mat_condition(lpgp_ctx* ctx, lpgp_mat* mat, int64_t n, const lpgp_pts* X_new, const lpgp_cond_block* row, int32_t nrow,
                       double noise_scalar, const double* noise_diag, const double* noise_dense, int32_t lazy, int32_t* info) {
  LPGP_CHECK(ctx && mat && row && n > 0, "lpgp_mat_condition: bad argument");
  LPGP_CHECK(nrow == (int32_t)mat->blocks.size() + 1, "lpgp_mat_condition: %d row entries for %d earlier blocks", nrow, (int)mat->blocks.size());
  LPGP_CHECK((noise_diag != nullptr) + (noise_dense != nullptr) + (noise_scalar != 0.0) <= 1, "lpgp_mat_condition: more than one form of noise");
  LPGP_CHECK(lazy == 0 || !ctx->distributed(), "lpgp_mat_condition: lazy status on a single GPU only");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_mat_condition");
  if (info) *info = 0;
  // earlier blocks that were only assembled (lazy == 2): another deferred block joins them -- they are factored TOGETHER by
  // whoever needs the factor first, one factorisation from the first unfactored column on (lpgp_potrf_predict: with the
  // prediction riding inside all of it); lazy == 1 enqueues their factorisation first, lazy == 0 requires them factored
  if (lazy == 1 && mat->pn_fact < mat->pn) LPGP_TRY(lpgp_potrf_enqueue(ctx, mat));
  LPGP_CHECK(lazy == 2 || mat->pn_fact == mat->pn, "lpgp_mat_condition: earlier blocks are not factored (lpgp_potrf first)");
  // (the identity tail of the block is written by ONE launch together with its noise, behind the assembly -- fused_finish;
  //  the assembly kernels touch logical entries only)
  const bool fused_finish = ctx->asm_batch && !noise_dense;
  const int bi = mat_add_block_impl(ctx, mat, n, !fused_finish);
  if (bi < 0) return bi;
  PopBlock undo{ctx, mat};
  const lpgp_block B = mat->blocks[bi];
  // the block row with as few launches as it has DIFFERENT descriptors; without `asm_batch`, or in a multi-GPU job, entry by entry
  const bool batch = ctx->asm_batch && !ctx->distributed();
  AsmRun run{ctx, mat->a, mat->lr_cap, mat_layout(ctx)};
  DevDesc desc;
  for (int j = 0; j < nrow; ++j) {
    const lpgp_cond_block& e = row[j];
    if (e.F0) {
      LPGP_TRY(run.flush());
      LPGP_TRY(lpgp_gram_assemble_grid(ctx, e.kd, e.ngroups, e.F0, j == bi ? nullptr : e.F1, mat, bi, j));
      continue;
    }
    const lpgp_pts* Xc = (j == bi) ? X_new : e.X1;
    const lpgp_block& Bj = mat->blocks[j];
    LPGP_CHECK(X_new && Xc && e.kd, "lpgp_mat_condition: null point set or descriptor in row entry %d", j);
    LPGP_CHECK(X_new->n == B.n && Xc->n == Bj.n && Xc->d == X_new->d && e.kd[0].d == X_new->d, "lpgp_mat_condition: shape mismatch in row entry %d", j);
    LPGP_TRY(lower_kdesc(e.kd, e.ngroups, &desc));
    LPGP_TRY(run.add(desc, AsmJob{X_new->x, X_new->n, X_new->n_pad, Xc->x, Xc->n, Xc->n_pad, B.poff, Bj.poff, j == bi ? 1 : 0}));
    if (!batch) LPGP_TRY(run.flush());
  }
  LPGP_TRY(run.flush());
  if (noise_scalar != 0.0 && !fused_finish) LPGP_TRY(lpgp_mat_add_diag(ctx, mat, bi, nullptr, noise_scalar));
  if (noise_dense) LPGP_TRY(lpgp_mat_add_dense(ctx, mat, bi, noise_dense));
  if (fused_finish && !noise_diag) LPGP_TRY(finish_block(ctx, mat, B, noise_scalar != 0.0 ? B.n : 0, nullptr, noise_scalar));
  if (noise_diag) {
    // the vector is staged into the block's own segment of the weights buffer (unused until the first solve, which is
    // stream-ordered behind the kernel below) through a stream that is idle during conditionings: nothing waits for the
    // panel stream, where an enqueued factorisation of the previous block may still be running
    // (only while an enqueued factorisation is in flight -- `unchecked` -- is the side stream worth anything; otherwise the
    //  panel stream, which orders the upload behind whatever a caller of the C API left running on it: lpgp.h, "streams")
    hipStream_t sc = (mat->unchecked && ctx->s_upd_all && !ctx->single_stream && !ctx->distributed()) ? ctx->s_upd_all : ctx->s_main;
    hipError_t e = hipMemcpyAsync(mat->w + B.poff, noise_diag, (size_t)B.n * sizeof(double), hipMemcpyHostToDevice, sc);
    if (e == hipSuccess) e = hipStreamSynchronize(sc);
    LPGP_CHECK(e == hipSuccess, "lpgp_mat_condition: noise upload: %s", hipGetErrorString(e));
    if (fused_finish) LPGP_TRY(finish_block(ctx, mat, B, B.n, mat->w + B.poff, 0.0));
    else LPGP_TRY(launch_add_diag(ctx->s_main, mat->a, mat->lr_cap, B.poff, B.n, mat->w + B.poff, 0.0, mat_layout(ctx)));
  }
  int32_t h = 0;
  // lazy == 2: the block row is assembled and the factorisation is left to whoever needs the factor first -- the next
  // lpgp_mat_condition / lpgp_potrf / lpgp_potrf_enqueue, or lpgp_potrf_predict, which lets the prediction ride inside it
  if (lazy != 2) LPGP_TRY(lazy ? lpgp_potrf_enqueue(ctx, mat) : lpgp_potrf(ctx, mat, &h));
  if (info) *info = h;
  undo.armed = (h != 0);           // (a factorisation that found the matrix not positive definite: status reported, block dropped)
  return 0;
}

int lpgp_mat_check(lpgp_ctx* ctx, lpgp_mat* mat, int32_t* info, int32_t* block) {
  LPGP_CHECK(ctx && mat && info, "lpgp_mat_check: null argument");
  LPGP_DEVICE(ctx);
  *info = 0;
  if (block) *block = -1;
  if (!mat->unchecked) return 0;
  int h = 0;
  if (mat->status_known) {
    h = mat->status_value;             // read back by lpgp_potrf_predict together with its results, nothing enqueued since
  } else {
    LPGP_HIP(hipMemcpyAsync(&h, mat->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->s_main));
    LPGP_HIP(hipStreamSynchronize(ctx->s_main));
  }
  mat->take_status(h);               // (h < 0 poisons the matrix: the status word stays at INT_MIN)
  LPGP_CHECK(h >= 0, "resident panel chain: a hand-over between workgroups timed out (device status %d); set LPGP_CHAIN_RESIDENT=-1", h);
  *info = h;
  if (h > 0 && block) *block = mat->block_of_pivot(h);
  return 0;
}

int lpgp_mat_truncate(lpgp_ctx* ctx, lpgp_mat* mat, int32_t nblocks) {
  LPGP_CHECK(ctx && mat, "lpgp_mat_truncate: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(mat->hidden.empty(), "lpgp_mat_truncate: a strict prefix of the blocks is in view");
  LPGP_CHECK(nblocks >= 0 && nblocks <= (int32_t)mat->blocks.size(), "lpgp_mat_truncate: %d of %d blocks", nblocks, (int)mat->blocks.size());
  LPGP_CHECK(!ctx->distributed(), "lpgp_mat_truncate: single GPU only");
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));        // nothing of the dropped blocks still in flight
  LPGP_HIP(hipMemset(mat->d_status, 0, sizeof(int)));
  mat->truncate(nblocks);
  return 0;
}

int lpgp_potrs(lpgp_ctx* ctx, lpgp_mat* mat, double* b_host, int64_t nrhs) {
  LPGP_CHECK(ctx && mat && b_host && nrhs >= 1, "lpgp_potrs: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_potrs");
  LPGP_CHECK(mat->pn_fact == mat->pn && mat->pn > 0, "lpgp_potrs: matrix is not factored");
  const int64_t pn = mat->pn, n = mat->n, m_pad = round_up(nrhs, TILE);
  std::vector<double> hp((size_t)pn * m_pad, 0.0);
  DevBuf dv;                                     // (released by hipFree, which waits for the device: behind hp, so in front of it on the way out)
  LPGP_TRY(DevBuf::raw(hp.size() * sizeof(double), &dv));
  for (int64_t j = 0; j < nrhs; ++j) mat->scatter_padded(b_host + j * n, hp.data() + j * pn);
  LPGP_HIP(hipMemcpyAsync(dv.as(), hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->s_main));
  LPGP_TRY(solve_lower(ctx, mat, dv.as(), pn, m_pad));
  LPGP_TRY(solve_lower_t(ctx, mat, dv.as(), pn, m_pad));
  // (wait FIRST, watched: the copy into pageable memory below is synchronous and would wait unwatched behind a streamed
  //  solve whose peer is gone)
  LPGP_TRY(sync_stream(ctx, ctx->s_main));
  LPGP_HIP(hipMemcpyAsync(hp.data(), dv.as(), hp.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
  LPGP_TRY(sync_stream(ctx, ctx->s_main));       // (behind a streamed solve: polls, so that a failed peer cannot block this rank)
  for (int64_t j = 0; j < nrhs; ++j) mat->gather_padded(hp.data() + j * pn, b_host + j * n);
  return 0;
}

// multi-GPU form of lpgp_solve_weights: the factor is streamed; the vector rides as column 0 of a 128-column block on every
// rank (all ranks end with the same weights, no further communication)
static int solve_weights_dist(lpgp_ctx* ctx, lpgp_mat* mat) {
  const int64_t pn = mat->pn;
  const size_t vb = (size_t)pn * TILE * sizeof(double);
  DevBuf dv;
  LPGP_TRY(DevBuf::pool(ctx, vb, &dv));
  LPGP_HIP(hipMemsetAsync(dv.as(), 0, vb, ctx->s_main));
  LPGP_HIP(hipMemcpyAsync(dv.as(), mat->w, (size_t)pn * sizeof(double), hipMemcpyDeviceToDevice, ctx->s_main));
  LPGP_TRY(solve_lower(ctx, mat, dv.as(), pn, TILE));
  LPGP_TRY(solve_lower_t(ctx, mat, dv.as(), pn, TILE));
  LPGP_HIP(hipMemcpyAsync(mat->w, dv.as(), (size_t)pn * sizeof(double), hipMemcpyDeviceToDevice, ctx->s_main));
  return 0;
}

int lpgp_solve_weights(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, double* w_host) {
  LPGP_CHECK(ctx && mat && r_host, "lpgp_solve_weights: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_solve_weights");
  LPGP_CHECK(mat->pn_fact == mat->pn && mat->pn > 0, "lpgp_solve_weights: matrix is not factored");
  const int64_t pn = mat->pn;
  LPGP_TRY(ensure_tmp(ctx, pn + 2));                // (+ 2: the ticket words of the resident solve, trsv.hip)
  // through pinned staging: the residual up and the weights + the solve's status word back are asynchronous copies, ONE wait
  // (round 6; until then two blocking copies through pageable memory around 2 x T dependent launches)
  LPGP_TRY(ensure_stage(ctx, pn));
  double* const hs = ctx->h_stage;
  int* const hinfo = ctx->h_info_pinned + lpgp_ctx::PIN_SOLVE_WEIGHTS;
  mat->scatter_padded(r_host, hs);
  LPGP_HIP(hipMemcpyAsync(mat->w, hs, (size_t)pn * sizeof(double), hipMemcpyHostToDevice, ctx->s_main));
  if (ctx->distributed()) {
    LPGP_TRY(dist_fail(ctx, solve_weights_dist(ctx, mat)));     // (any failure: the peers are inside the streamed solve, or about to enter it)
    *hinfo = 0;
    LPGP_TRY(sync_stream(ctx, ctx->s_main));      // (watched: a copy behind a streamed solve whose peer is gone would wait for ever)
  } else {
    FactorView F;
    LPGP_TRY(factor_view(mat, &F));
    LPGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), ctx->s_main));
    LPGP_TRY(solve_vec(ctx, F, pn / TILE, mat->w, ctx->d_tmp, ctx->d_info));
    LPGP_HIP(hipMemcpyAsync(hinfo, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, ctx->s_main));
  }
  LPGP_HIP(hipMemcpyAsync(hs, mat->w, (size_t)pn * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
  LPGP_TRY(sync_stream(ctx, ctx->s_main));
  LPGP_CHECK(*hinfo >= 0, "resident single-vector solve: a hand-over between workgroups timed out (device status %d); set LPGP_TRSV_RESIDENT=0", *hinfo);
  mat->weights_resident();
  if (w_host) mat->gather_padded(hs, w_host);
  return 0;
}

int lpgp_mat_set_residual(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host) {
  LPGP_CHECK(ctx && mat && r_host, "lpgp_mat_set_residual: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(mat->pn > 0, "lpgp_mat_set_residual: empty matrix");      // (factored or not: lpgp_potrf_predict takes it along)
  if (!ctx->distributed() && !ctx->single_stream) {
    // Through pinned staging on the panel stream, NO wait (round 5): every reader of the residual is a kernel or a copy on the
    // panel stream (lpgp_predict, lpgp_potrf_predict, lpgp_solve_weights), the caller's vector has been consumed when this
    // returns; the staging buffer is reused only after the previous upload has completed (an event, long signalled when the
    // next call comes).  Until round 5: a copy from pageable memory on a side stream and a wait for it, ~15 us of a host that a
    // small problem's step is bound by.
    if (ctx->stage_r_cap < mat->pn) {
      if (ctx->h_stage_r) {
        LPGP_HIP(hipEventSynchronize(ctx->ev_stage_r));
        LPGP_HIP(hipHostFree(ctx->h_stage_r));
      }
      ctx->h_stage_r = nullptr;
      ctx->stage_r_cap = 0;
      LPGP_HIP(hipHostMalloc(&ctx->h_stage_r, (size_t)mat->pn * sizeof(double), hipHostMallocDefault));
      ctx->stage_r_cap = mat->pn;
      if (!ctx->ev_stage_r) LPGP_HIP(hipEventCreateWithFlags(&ctx->ev_stage_r, hipEventDisableTiming));
    } else {
      LPGP_HIP(hipEventSynchronize(ctx->ev_stage_r));
    }
    mat->scatter_padded(r_host, ctx->h_stage_r);
    LPGP_HIP(hipMemcpyAsync(mat->r(), ctx->h_stage_r, (size_t)mat->pn * sizeof(double), hipMemcpyHostToDevice, ctx->s_main));
    LPGP_HIP(hipEventRecord(ctx->ev_stage_r, ctx->s_main));
    mat->residual_resident();
    return 0;
  }
  LPGP_CHECK(mat->pn_fact == mat->pn, "lpgp_mat_set_residual: matrix is not factored");      // (this branch has no lpgp_potrf_predict to consume an unfactored one)
  std::vector<double> hp((size_t)mat->pn);
  mat->scatter_padded(r_host, hp.data());
  // NOT on the panel stream: the residual's place in HBM is touched by no kernel of the factorisation, so the upload need
  // not queue behind an enqueued factorisation (lpgp_potrf_enqueue); it is complete when this call returns.  The update
  // stream of the blocked solves is idle whenever this is called (its work is joined into the panel stream at the end of
  // every solve) -- and it is an EXISTING stream: HIP multiplexes streams over four hardware queues, and a fifth stream
  // made two of them share one (measured: c2 predict 2.8 -> 5.6 ms).
  hipStream_t sc = (mat->unchecked && ctx->s_upd_all && !ctx->single_stream) ? ctx->s_upd_all : ctx->s_main;
  LPGP_HIP(hipMemcpyAsync(mat->r(), hp.data(), (size_t)mat->pn * sizeof(double), hipMemcpyHostToDevice, sc));
  LPGP_HIP(hipStreamSynchronize(sc));
  mat->residual_resident();
  return 0;
}

// ---- prediction -----------------------------------------------------------------------------
// What lpgp_rhs_create has to clear -- the rows of the blocks' padding tails (all logical columns) and the spare columns (all
// rows) -- in ONE launch (until round 5: a memset for the spare columns and a 2-D memset per padded block; five launches in
// front of every prediction of the reference's 2-D Poisson problem).  Job j < nj: rows [row0[j], row0[j] + nr[j]) x m columns;
// job nj: ld x (m_pad - m) doubles from column m on.
constexpr int RHS_PAD_JOBS = 15;
struct RhsPadJobs { int64_t row0[RHS_PAD_JOBS]; int32_t nr[RHS_PAD_JOBS]; int32_t nj; };
__global__ void rhs_pad_kernel(double* v, int64_t ld, int64_t m, int64_t m_pad, RhsPadJobs jb, int spare) {
  const int j = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j < jb.nj) {
    const int64_t nr = jb.nr[j], tot = nr * m;
    double* p = v + jb.row0[j];
    for (int64_t t = t0; t < tot; t += stride) p[(t % nr) + (t / nr) * ld] = 0.0;
  } else if (spare) {
    const int64_t tot = ld * (m_pad - m);
    double* p = v + ld * m;
    for (int64_t t = t0; t < tot; t += stride) p[t] = 0.0;
  }
}

// a right-hand side of ld rows x m columns: allocated (contents undefined) and counted in live_mats
static int rhs_new(lpgp_ctx* ctx, int64_t ld, int64_t m, std::unique_ptr<lpgp_rhs, Destroy>* out) {
  const int64_t m_pad = round_up(m + 1, TILE);       // at least one spare column (see lpgp_predict)
  DevBuf v;
  LPGP_TRY(DevBuf::pool(ctx, (size_t)ld * m_pad * sizeof(double), &v));
  lpgp_rhs* r = new lpgp_rhs();
  r->ctx = ctx;
  r->ld = ld;
  r->m = m;
  r->m_pad = m_pad;
  r->v = (double*)v.release();
  ++ctx->live_mats;
  out->reset(r);
  return 0;
}

int lpgp_rhs_create(lpgp_ctx* ctx, const lpgp_mat* mat, int64_t m, lpgp_rhs** out) {
  LPGP_CHECK(ctx && mat && out && m >= 1, "lpgp_rhs_create: bad argument");
  LPGP_DEVICE(ctx);
  std::unique_ptr<lpgp_rhs, Destroy> r;
  LPGP_TRY(rhs_new(ctx, mat->pn, m, &r));
  // lpgp_cross_assemble writes every logical row of every logical column: only the spare columns and
  // the rows of the blocks' padding tails have to be cleared (c3: 17 MB instead of 571 MB per prediction)
  {
    RhsPadJobs jb;
    jb.nj = 0;
    int spare = 1;
    int64_t work = r->ld * (r->m_pad - m);
    auto flush = [&]() {
      const int64_t wgs = (work + 2047) / 2048;
      hipLaunchKernelGGL(rhs_pad_kernel, dim3((unsigned)(wgs < 1 ? 1 : (wgs > 2048 ? 2048 : wgs)), (unsigned)(jb.nj + spare)), dim3(256), 0, ctx->s_main,
                         r->v, r->ld, m, r->m_pad, jb, spare);
      jb.nj = 0;
      spare = 0;
      work = 0;
    };
    for (const auto& b : mat->blocks)
      if (b.pn > b.n) {
        jb.row0[jb.nj] = b.poff + b.n;
        jb.nr[jb.nj] = (int32_t)(b.pn - b.n);
        ++jb.nj;
        work = std::max(work, (int64_t)(b.pn - b.n) * m);
        if (jb.nj == RHS_PAD_JOBS) flush();
      }
    if (jb.nj > 0 || spare) flush();
    LPGP_HIP(hipGetLastError());
  }
  r->assembled.assign(mat->blocks.size(), 0);
  *out = r.release();
  return 0;
}

// rows of observation blocks that were never assembled count as zero cross-covariance
static int rhs_clear_unassembled(lpgp_ctx* ctx, const lpgp_mat* mat, lpgp_rhs* r) {
  for (size_t bi = 0; bi < r->assembled.size() && bi < mat->blocks.size(); ++bi) {
    if (r->assembled[bi]) continue;
    const lpgp_block& b = mat->blocks[bi];
    if (b.n > 0)
      LPGP_HIP(hipMemset2DAsync(r->v + b.poff, (size_t)r->ld * sizeof(double), 0, (size_t)b.n * sizeof(double), (size_t)r->m,
                                ctx->s_main));
    r->assembled[bi] = 1;
  }
  return 0;
}

int lpgp_rhs_destroy(lpgp_rhs* r) {
  if (!r) return 0;
  (void)hipSetDevice(r->ctx->device);
  pool_free(r->ctx, r->v, (size_t)r->ld * r->m_pad * sizeof(double));
  --r->ctx->live_mats;
  delete r;
  return 0;
}

// What the lpgp_cross_assemble* entry points ask of their target: the handles there (tested before any is read), blocks
// [bi, bi + nb) of the matrix, and a right-hand side made for this matrix and these test points.
static int cross_target(const char* fn, const lpgp_pts* X_test, const lpgp_rhs* rhs, const lpgp_mat* mat, int32_t bi, int32_t nb) {
  LPGP_CHECK(X_test && rhs && mat, "%s: null argument", fn);
  LPGP_CHECK(bi >= 0 && nb >= 0 && bi + nb <= (int)mat->blocks.size(), "%s: bad block %d", fn, bi);
  LPGP_CHECK(rhs->ld == mat->pn, "%s: rhs was created for a different matrix size", fn);
  LPGP_CHECK(X_test->n == rhs->m, "%s: shape mismatch: X_test has %lld points, rhs has %lld columns", fn, (long long)X_test->n, (long long)rhs->m);
  return 0;
}

int lpgp_cross_assemble(lpgp_ctx* ctx, const lpgp_kdesc* kd, int32_t ngroups, const lpgp_pts* X_obs,
                        const lpgp_pts* X_test, lpgp_rhs* rhs, const lpgp_mat* mat, int32_t bi) {
  LPGP_CHECK(ctx && kd && X_obs, "lpgp_cross_assemble: null argument");
  LPGP_DEVICE(ctx);
  LPGP_TRY(cross_target("lpgp_cross_assemble", X_test, rhs, mat, bi, 1));
  const lpgp_block& B = mat->blocks[bi];
  LPGP_CHECK(X_obs->n == B.n && X_obs->d == X_test->d && kd[0].d == X_obs->d, "lpgp_cross_assemble: shape mismatch");
  DevDesc desc;
  int rc = lower_kdesc(kd, ngroups, &desc);
  if (rc != 0) return rc;
  rc = launch_assemble(ctx, ctx->s_main, desc, X_obs->x, X_obs->n, X_obs->n_pad, X_test->x, X_test->n,
                       X_test->n_pad, rhs->v, rhs->ld, B.poff, 0, 0);
  if (rc == 0 && bi < (int)rhs->assembled.size()) rhs->assembled[bi] = 1;
  return rc;       // asynchronous (see lpgp_gram_assemble)
}

int lpgp_cross_assemble_weighted(lpgp_ctx* ctx, const lpgp_wpair* pairs, int32_t npairs, const double* w_host, int32_t A,
                                 const lpgp_pts* X_obs, const lpgp_pts* X_test, lpgp_rhs* rhs, const lpgp_mat* mat, int32_t bi) {
  static const char* fn = "lpgp_cross_assemble_weighted";
  LPGP_CHECK(ctx && X_obs, "%s: null argument", fn);
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "%s: single GPU only (this context has joined a multi-GPU job)", fn);
  LPGP_TRY(cross_target(fn, X_test, rhs, mat, bi, 1));
  const lpgp_block& B = mat->blocks[bi];
  LPGP_CHECK(w_host != nullptr, "%s: null weights", fn);
  LPGP_TRY_RC(check_wpairs(pairs, npairs, A, 1, WP_CROSS, fn));
  LPGP_CHECK(X_obs->n == B.n && X_obs->d == X_test->d && pairs[0].kd[0].d == X_obs->d, "%s: shape mismatch", fn);
  int rc = 0;
  if (X_test->n > 0 && X_obs->n > 0) {
    const std::vector<double> ones((size_t)X_test->n, 1.0);
    rc = assemble_weighted(ctx, ctx->s_main, pairs, npairs, w_host, A, ones.data(), 1, X_obs, X_test, false, rhs->v, rhs->ld, B.poff, 0, Layout2D());
  }
  if (rc == 0 && bi < (int)rhs->assembled.size()) rhs->assembled[bi] = 1;
  return rc;
}

int lpgp_cross_assemble_mixed(lpgp_ctx* ctx, const lpgp_kdesc* kd, int32_t ngroups, const lpgp_pts* X_obs, const lpgp_mix* M,
                              const lpgp_pts* X_test, lpgp_rhs* rhs, const lpgp_mat* mat, int32_t bi) {
  static const char* fn = "lpgp_cross_assemble_mixed";
  LPGP_CHECK(ctx && kd && X_obs, "%s: null argument", fn);
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "%s: single GPU only (this context has joined a multi-GPU job)", fn);
  LPGP_TRY(cross_target(fn, X_test, rhs, mat, bi, 1));
  LPGP_CHECK(rhs->ctx == ctx && mat->ctx == ctx && X_test->ctx == ctx, "%s: a handle belongs to another context", fn);
  int64_t rows = 0;
  LPGP_TRY(mix_side(fn, ctx, X_obs, M, "observation", &rows));
  const lpgp_block& B = mat->blocks[bi];
  LPGP_CHECK(rows == B.n, "%s: the observation side has %lld rows, block %d has %lld", fn, (long long)rows, bi, (long long)B.n);
  LPGP_CHECK(X_obs->d == X_test->d && kd[0].d == X_obs->d, "%s: dimension mismatch", fn);
  DevDesc desc;
  LPGP_TRY(lower_kdesc(kd, ngroups, &desc));
  int rc = 0;
  if (X_test->n > 0) rc = assemble_mixed(ctx, ctx->s_main, desc, X_obs, M, X_test, nullptr, false, rhs->v, rhs->ld, B.poff, 0, Layout2D());
  if (rc == 0 && bi < (int)rhs->assembled.size()) rhs->assembled[bi] = 1;
  return rc;       // asynchronous (see lpgp_gram_assemble)
}

int lpgp_cross_assemble_row(lpgp_ctx* ctx, const lpgp_cross_block* blocks, int32_t nblocks, const lpgp_pts* X_test, lpgp_rhs* rhs,
                            const lpgp_mat* mat) {
  LPGP_CHECK(ctx && blocks, "lpgp_cross_assemble_row: null argument");
  LPGP_DEVICE(ctx);
  LPGP_TRY(cross_target("lpgp_cross_assemble_row", X_test, rhs, mat, 0, nblocks));
  LPGP_CHECK(nblocks == (int32_t)mat->blocks.size(), "lpgp_cross_assemble_row: %d entries for %d blocks", nblocks, (int)mat->blocks.size());
  AsmRun run{ctx, rhs->v, rhs->ld, Layout2D(), &rhs->assembled};
  DevDesc desc;
  for (int bi = 0; bi < nblocks; ++bi) {
    const lpgp_cross_block& e = blocks[bi];
    const lpgp_block& B = mat->blocks[(size_t)bi];
    if (!e.kd || !e.X_obs) continue;                       // a block without cross-covariance: its rows stay zero (rhs_clear_unassembled)
    LPGP_CHECK(e.X_obs->n == B.n && e.X_obs->d == X_test->d && e.kd[0].d == X_test->d, "lpgp_cross_assemble_row: shape mismatch in block %d", bi);
    LPGP_TRY(lower_kdesc(e.kd, e.ngroups, &desc));
    LPGP_TRY(run.add(desc, AsmJob{e.X_obs->x, e.X_obs->n, e.X_obs->n_pad, X_test->x, X_test->n, X_test->n_pad, B.poff, 0, 0}, bi));
  }
  return run.flush();       // asynchronous (see lpgp_gram_assemble)
}

int lpgp_trsm_lower(lpgp_ctx* ctx, lpgp_mat* mat, lpgp_rhs* V) {
  LPGP_CHECK(ctx && mat && V, "lpgp_trsm_lower: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_trsm_lower");
  LPGP_CHECK(mat->pn_fact == mat->pn && V->ld == mat->pn, "lpgp_trsm_lower: matrix not factored or size mismatch");
  LPGP_TRY(rhs_clear_unassembled(ctx, mat, V));
  LPGP_TRY(solve_lower(ctx, mat, V->v, V->ld, V->m_pad));
  LPGP_TRY(sync_stream(ctx, ctx->s_main));
  return 0;
}

// The read-back tail of a prediction: the column reductions of K (dots with `dot`, if given; sums of squares, if `squares`) into
// d_tmp, ONE asynchronous copy of them into the pinned staging buffer -- and one of the matrix's status word into `h_status`,
// if given -- ONE watched wait, then  mean = prior_mean + dots,  var = kxx - squares.
static int reduce_read_back(lpgp_ctx* ctx, const lpgp_mat* mat, const lpgp_rhs* K, const double* dot, bool squares, const double* prior_mean_host,
                            const double* kxx_host, double* mean_host, double* var_host, int* h_status) {
  const int64_t m = K->m, sq0 = dot && squares ? K->m_pad : 0;
  if (dot && squares)
    hipLaunchKernelGGL(col_reduce2_kernel, dim3((unsigned)m), dim3(256), 0, ctx->s_main, K->v, K->ld, mat->pn, dot, ctx->d_tmp, ctx->d_tmp + sq0);
  else
    hipLaunchKernelGGL(col_reduce_kernel, dim3((unsigned)m), dim3(256), 0, ctx->s_main, K->v, K->ld, mat->pn, dot, ctx->d_tmp);
  LPGP_HIP(hipGetLastError());
  double* const hs = ctx->h_stage;
  LPGP_HIP(hipMemcpyAsync(hs, ctx->d_tmp, (size_t)(sq0 + m) * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
  if (h_status) LPGP_HIP(hipMemcpyAsync(h_status, mat->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->s_main));
  LPGP_TRY(sync_stream(ctx, ctx->s_main));
  if (dot)
    for (int64_t j = 0; j < m; ++j) mean_host[j] = (prior_mean_host ? prior_mean_host[j] : 0.0) + hs[j];
  if (squares)
    for (int64_t j = 0; j < m; ++j) var_host[j] = kxx_host[j] - hs[sq0 + j];
  return 0;
}

int lpgp_predict(lpgp_ctx* ctx, lpgp_mat* mat, lpgp_rhs* K, const double* prior_mean_host,
                 const double* kxx_host, double* mean_host, double* var_host) {
  LPGP_CHECK(ctx && mat && K, "lpgp_predict: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_predict");
  LPGP_CHECK(mat->pn_fact == mat->pn && K->ld == mat->pn, "lpgp_predict: matrix not factored or size mismatch");
  LPGP_TRY(ensure_tmp(ctx, 2 * K->m_pad));
  LPGP_TRY(rhs_clear_unassembled(ctx, mat, K));
  // results come back through pinned staging: the copy is asynchronous (the one wait polls, so that a failed peer of a
  // multi-GPU job cannot block this rank inside a copy) and mean + variance are ONE copy, not two blocking round trips
  LPGP_TRY(ensure_stage(ctx, 2 * K->m_pad));
  // Mean and variance together: the variance needs V = L^{-1} K_Xx anyway, and
  //   K_xX G^{-1} r = V^T z  with  z = L^{-1} r,
  // so no representer weights are needed: the residual rides through the blocked solve as
  // the spare column m of the right-hand side (a side-stream triangular solve for z was
  // measured instead: its 132 dependent launches queue behind the resident GEMM workgroups
  // and stretch the step from 68 to 100 ms).
  const bool via_z = mean_host && var_host && !mat->has_w && mat->has_r;
  if (mean_host && !via_z) {
    LPGP_CHECK(mat->has_w, "lpgp_predict: representer weights not computed (call lpgp_solve_weights%s)",
               var_host ? " or lpgp_mat_set_residual" : "");
    LPGP_TRY(reduce_read_back(ctx, mat, K, mat->w, false, prior_mean_host, nullptr, mean_host, nullptr, nullptr));
  }
  if (var_host) {
    LPGP_CHECK(kxx_host != nullptr, "lpgp_predict: kxx_host required for the variance");
    double* zcol = K->v + (int64_t)K->m * K->ld;
    if (via_z)
      LPGP_HIP(hipMemcpyAsync(zcol, mat->r(), (size_t)mat->pn * sizeof(double), hipMemcpyDeviceToDevice, ctx->s_main));
    LPGP_TRY(solve_lower(ctx, mat, K->v, K->ld, K->m_pad));
    LPGP_TRY(reduce_read_back(ctx, mat, K, via_z ? zcol : nullptr, true, prior_mean_host, kxx_host, mean_host, var_host, nullptr));
  }
  return 0;
}

int lpgp_potrf_predict(lpgp_ctx* ctx, lpgp_mat* mat, lpgp_rhs* K, const double* prior_mean_host, const double* kxx_host,
                       double* mean_host, double* var_host) {
  LPGP_CHECK(ctx && mat && K && kxx_host && mean_host && var_host, "lpgp_potrf_predict: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_potrf_predict");
  LPGP_CHECK(!ctx->distributed(), "lpgp_potrf_predict: single GPU only (a multi-GPU job factors collectively: lpgp_potrf, lpgp_predict)");
  LPGP_CHECK(mat->hidden.empty(), "lpgp_potrf_predict: a strict prefix of the blocks is in view");
  LPGP_CHECK(K->ld == mat->pn && mat->pn > 0, "lpgp_potrf_predict: right-hand side built for another matrix size");
  LPGP_CHECK(mat->has_r, "lpgp_potrf_predict: no residual resident (lpgp_mat_set_residual)");
  LPGP_TRY(ensure_tmp(ctx, 2 * K->m_pad));
  LPGP_TRY(ensure_stage(ctx, 2 * K->m_pad));
  LPGP_TRY(rhs_clear_unassembled(ctx, mat, K));
  double* zcol = K->v + (int64_t)K->m * K->ld;          // the residual rides as the spare column: z = L^{-1} r, mean = V^T z
  LPGP_HIP(hipMemcpyAsync(zcol, mat->r(), (size_t)mat->pn * sizeof(double), hipMemcpyDeviceToDevice, ctx->s_main));
  const bool fresh = mat->pn_fact < mat->pn;
  const int rc = potrf_predict_blocked(ctx, mat, mat->pn_fact / TILE, mat->pn / TILE, K->v, K->ld, K->m_pad);
  if (rc != 0) {
    if (fresh) mat->poison();        // (partly factored in place with pn_fact unchanged -- a retry would factor a half-factored matrix)
    return rc;
  }
  if (fresh) mat->factor_enqueued(true);     // (provisionally, as lpgp_potrf_enqueue; the residual that rode along stays resident)
  mat->status_stale();
  // mean, variance and the status word of the factorisation come back together: two asynchronous copies into pinned memory,
  // ONE wait (until round 5: two blocking copies into pageable memory here and a third in lpgp_mat_check, ~25 us each --
  // a tenth of a step of the reference's own problem sizes)
  int* const hinfo = ctx->h_info_pinned + lpgp_ctx::PIN_POTRF_PREDICT;
  LPGP_TRY(reduce_read_back(ctx, mat, K, zcol, true, prior_mean_host, kxx_host, mean_host, var_host, hinfo));
  mat->status_read_back(*hinfo);
  return 0;
}

int lpgp_rhs_inner(lpgp_ctx* ctx, lpgp_rhs* A, lpgp_rhs* B, double* out_host) {
  LPGP_CHECK(ctx && A && B && out_host, "lpgp_rhs_inner: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(A->ld == B->ld, "lpgp_rhs_inner: row mismatch");
  const int64_t ma = A->m_pad, mb = B->m_pad;
  std::vector<double> h((size_t)ma * mb);
  DevBuf dc;
  LPGP_TRY(DevBuf::raw(h.size() * sizeof(double), &dc));
  StreamDrain drain{ctx->s_main};
  LPGP_TRY(launch_gemm(ctx, ctx->s_main, 1, 1, mk(A->v, A->ld, B->v, B->ld, dc.as(), ma, (int)(ma / TILE), (int)(mb / TILE), (int)A->ld, 1.0, 0.0, 0),
                       LPGP_K_GEMM));
  LPGP_HIP(hipMemcpyAsync(h.data(), dc.as(), h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
  LPGP_TRY(drain.wait());
  for (int64_t i = 0; i < A->m; ++i)
    for (int64_t j = 0; j < B->m; ++j) out_host[i * B->m + j] = h[(size_t)(i + j * ma)];
  return 0;
}

int lpgp_rhs_matmul(lpgp_ctx* ctx, const lpgp_rhs* A, const double* B_host, int64_t m, lpgp_rhs** out_new) {
  LPGP_CHECK(ctx && A && B_host && out_new && m >= 1, "lpgp_rhs_matmul: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "lpgp_rhs_matmul: single GPU only");
  // the result shares A's row layout whatever the matrix A was created for has become since (a posterior is a value: later
  // conditionings extend the shared matrix); every element of it is written by the product (beta = 0): no clearing
  std::unique_ptr<lpgp_rhs, Destroy> out;
  LPGP_TRY(rhs_new(ctx, A->ld, m, &out));
  out->assembled.assign(A->assembled.size(), 1);
  const int64_t ka = A->m_pad, mp = out->m_pad;
  // B, zero-padded to (columns of A incl. its spare ones) x (columns of out incl. its spare ones), column-major: the spare
  // columns of A meet zero rows, the spare columns of out come out as zeros
  std::vector<double> hb((size_t)ka * mp, 0.0);
  for (int64_t kk = 0; kk < A->m; ++kk)
    for (int64_t j = 0; j < m; ++j) hb[(size_t)(kk + j * ka)] = B_host[kk * m + j];
  const size_t bb = hb.size() * sizeof(double);
  DevBuf b;
  LPGP_TRY(DevBuf::pool(ctx, bb, &b));
  StreamDrain drain{ctx->s_main};                // (the staging vector is borrowed by the copy)
  LPGP_HIP(hipMemcpyAsync(b.as(), hb.data(), bb, hipMemcpyHostToDevice, ctx->s_main));
  LPGP_TRY(launch_gemm(ctx, ctx->s_main, 0, 1,
                       mk(A->v, A->ld, b.as(), ka, out->v, out->ld, (int)(out->ld / TILE), (int)(mp / TILE), (int)ka, 1.0, 0.0, 0), LPGP_K_GEMM));
  LPGP_TRY(drain.wait());
  *out_new = out.release();
  return 0;
}

int lpgp_mat_sub_inner(lpgp_ctx* ctx, lpgp_mat* S, int32_t bi, lpgp_rhs* V) {
  LPGP_CHECK(ctx && S && V, "lpgp_mat_sub_inner: null argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(S, "lpgp_mat_sub_inner");
  LPGP_CHECK(!ctx->distributed(), "lpgp_mat_sub_inner: single GPU only");
  LPGP_CHECK(bi >= 0 && bi < (int)S->blocks.size(), "lpgp_mat_sub_inner: bad block %d", bi);
  const lpgp_block& B = S->blocks[(size_t)bi];
  LPGP_CHECK(B.poff >= S->pn_fact, "lpgp_mat_sub_inner: block %d is already factored", bi);
  LPGP_CHECK(V->m == B.n, "lpgp_mat_sub_inner: V has %lld columns, block %d has %lld rows", (long long)V->m, bi, (long long)B.n);
  LPGP_CHECK(V->ld % TILE == 0 && V->m_pad >= B.pn, "lpgp_mat_sub_inner: bad right-hand-side layout");
  // the columns of V behind the logical ones that the product reads (the spare column may hold L^{-1} r after a prediction)
  if (B.pn > V->m)
    LPGP_HIP(hipMemsetAsync(V->v + V->m * V->ld, 0, (size_t)((B.pn - V->m) * V->ld) * sizeof(double), ctx->s_main));
  // C[c0:, c0 : c0 + BW] -= V[:, c0:]^T V[:, c0 : c0 + BW], band by band: the triangular form of the product exists for
  // row-major operands only, bands of BW tile columns from the diagonal down do (1 + 1 / nbands) / 2 of the full square's work
  const int T = (int)(B.pn / TILE), BW = 4;
  double* const C0 = S->a + B.poff * (S->lr_cap + 1);
  for (int c0 = 0; c0 < T; c0 += BW) {
    const double* Vc = V->v + (int64_t)c0 * TILE * V->ld;
    LPGP_TRY(launch_gemm(ctx, ctx->s_main, 1, 1,
                         mk(Vc, V->ld, Vc, V->ld, C0 + (int64_t)c0 * TILE * (S->lr_cap + 1), S->lr_cap, T - c0, std::min(BW, T - c0), (int)V->ld, -1.0,
                            1.0, 0),
                         LPGP_K_GEMM));
  }
  return 0;        // asynchronous: consumers are ordered behind it on the main stream
}

int lpgp_mat_factor_matmul(lpgp_ctx* ctx, lpgp_mat* mat, const double* Z_host, int64_t s, const double* shift_host, double* out_host) {
  LPGP_CHECK(ctx && mat && Z_host && out_host && s >= 1, "lpgp_mat_factor_matmul: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_MAT_ALIVE(mat, "lpgp_mat_factor_matmul");
  LPGP_CHECK(!ctx->distributed(), "lpgp_mat_factor_matmul: single GPU only");
  LPGP_CHECK(mat->pn > 0 && mat->pn_fact == mat->pn, "lpgp_mat_factor_matmul: matrix is not (fully) factored");
  LPGP_CHECK(!mat->unchecked, "lpgp_mat_factor_matmul: the status of an enqueued factorisation has not been read (lpgp_mat_check)");
  return factor_matmul(ctx, mat, Z_host, s, shift_host, out_host);
}

// the state every entry point of evidence.hip asks for: the checks of lpgp_mat_factor_matmul
#define LPGP_EVIDENCE_READY(fn)                                                                                                             \
  LPGP_DEVICE(ctx);                                                                                                                         \
  LPGP_MAT_ALIVE(mat, fn);                                                                                                                  \
  LPGP_CHECK(!ctx->distributed(), fn ": single GPU only");                                                                                  \
  LPGP_CHECK(mat->pn > 0 && mat->pn_fact == mat->pn, fn ": matrix is not (fully) factored");                                                \
  LPGP_CHECK(!mat->unchecked, fn ": the status of an enqueued factorisation has not been read (lpgp_mat_check)")

int lpgp_mat_evidence(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, double out_host[2]) {
  LPGP_CHECK(ctx && mat && r_host && out_host, "lpgp_mat_evidence: null argument");
  LPGP_EVIDENCE_READY("lpgp_mat_evidence");
  return mat_evidence(ctx, mat, r_host, out_host);
}

int lpgp_mat_inverse_diag(lpgp_ctx* ctx, lpgp_mat* mat, double* out_host) {
  LPGP_CHECK(ctx && mat && out_host, "lpgp_mat_inverse_diag: null argument");
  LPGP_EVIDENCE_READY("lpgp_mat_inverse_diag");
  return mat_inverse_diag(ctx, mat, out_host);
}

int lpgp_mat_loo(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, const double* y_host, double* mean_host, double* var_host, double* logp_host) {
  LPGP_CHECK(ctx && mat && r_host && y_host && mean_host && var_host && logp_host, "lpgp_mat_loo: null argument");
  LPGP_EVIDENCE_READY("lpgp_mat_loo");
  return mat_loo(ctx, mat, r_host, y_host, mean_host, var_host, logp_host);
}

int lpgp_mat_inverse(lpgp_ctx* ctx, lpgp_mat* mat, lpgp_mat** out) {
  LPGP_CHECK(ctx && mat && out, "lpgp_mat_inverse: null argument");
  LPGP_EVIDENCE_READY("lpgp_mat_inverse");
  lpgp_mat* created = nullptr;
  LPGP_TRY(lpgp_mat_create(ctx, mat->pn, &created));
  std::unique_ptr<lpgp_mat, Destroy> m(created);
  m->adopt_layout(*mat);                         // (not factored: a plain symmetric matrix in the lower triangle)
  LPGP_TRY(mat_inverse_into(ctx, mat, m.get()));
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));   // (a failure of the device work is reported here, with the handle still owned)
  *out = m.release();
  return 0;
}

int lpgp_mat_evidence_grad(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, const lpgp_mat* dG, const double* r_host, double out_host[2]) {
  LPGP_CHECK(ctx && mat && ginv && dG && r_host && out_host, "lpgp_mat_evidence_grad: null argument");
  LPGP_EVIDENCE_READY("lpgp_mat_evidence_grad");
  LPGP_TRY(evidence_grad_layout(mat, ginv, "lpgp_mat_evidence_grad", "the inverse"));
  LPGP_TRY(evidence_grad_layout(mat, dG, "lpgp_mat_evidence_grad", "the derivative"));
  return mat_evidence_grad(ctx, mat, ginv, dG, r_host, out_host);
}

int lpgp_mat_evidence_grad_diag(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, int32_t bi, const double* v_host, double scalar,
                                const double* r_host, double out_host[2]) {
  LPGP_CHECK(ctx && mat && ginv && r_host && out_host, "lpgp_mat_evidence_grad_diag: null argument");
  LPGP_EVIDENCE_READY("lpgp_mat_evidence_grad_diag");
  LPGP_CHECK(bi >= 0 && bi < (int32_t)mat->blocks.size(), "lpgp_mat_evidence_grad_diag: bad block %d", bi);
  LPGP_TRY(evidence_grad_layout(mat, ginv, "lpgp_mat_evidence_grad_diag", "the inverse"));
  return mat_evidence_grad_diag(ctx, mat, ginv, bi, v_host, scalar, r_host, out_host);
}

int lpgp_mat_cv(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, const double* r_host, const double* y_host, const int32_t* fold_of, int32_t nfolds,
                double* mean_host, double* var_host, double* logp_host, double* cov_host) {
  LPGP_CHECK(ctx && mat && ginv && r_host && y_host && fold_of && mean_host && var_host && logp_host, "lpgp_mat_cv: null argument");
  LPGP_EVIDENCE_READY("lpgp_mat_cv");
  LPGP_CHECK(nfolds >= 1, "lpgp_mat_cv: %d folds", nfolds);
  LPGP_TRY(evidence_grad_layout(mat, ginv, "lpgp_mat_cv", "the inverse"));
  return mat_cv(ctx, mat, ginv, r_host, y_host, fold_of, nfolds, mean_host, var_host, logp_host, cov_host);
}
#undef LPGP_EVIDENCE_READY

int lpgp_gemm_host(lpgp_ctx* ctx, int32_t transa, int32_t transb, int64_t m, int64_t n, int64_t k, double alpha,
                   const double* A_host, const double* B_host, double beta, double* C_host) {
  LPGP_CHECK(ctx && A_host && B_host && C_host && m >= 1 && n >= 1 && k >= 1, "lpgp_gemm_host: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(!ctx->distributed(), "lpgp_gemm_host: single GPU only");
  // The kernel computes column-major  C' = op(A') op(B')  on whole 128 x 128 tiles.  A C-order m x n result is the column-major
  // n x m matrix C^T = op(B)^T op(A)^T in the same memory: A' = op(B)^T (n x k), B' = op(A)^T (k x m), both read in place --
  // a C-order k x n array IS column-major n x k (ta = 0), a C-order n x k one is its k-fastest form (ta = 1); likewise for B'.
  const int64_t np_ = round_up(n, TILE), mp = round_up(m, TILE), kp = round_up(k, 16);
  // zero-padded device images (rows beyond the logical extent must be zeros, not stale pool contents: 0 * NaN)
  const int64_t a_ld = transb ? kp : np_, a_cols = transb ? np_ : kp;     // A' image: leading dimension x columns
  const int64_t b_ld = transa ? mp : kp, b_cols = transa ? kp : mp;
  const int64_t a_src_ld = transb ? k : n, a_src_cols = transb ? n : k;   // the host array behind it, as column-major ld x cols
  const int64_t b_src_ld = transa ? m : k, b_src_cols = transa ? k : m;
  const size_t ab = (size_t)a_ld * a_cols * sizeof(double), bb = (size_t)b_ld * b_cols * sizeof(double), cb = (size_t)np_ * mp * sizeof(double);
  DevBuf pc, pb, pa;                             // (declared in reverse: they go back into the pool in the order a, b, c)
  LPGP_TRY(DevBuf::pool(ctx, ab, &pa));
  LPGP_TRY(DevBuf::pool(ctx, bb, &pb));
  LPGP_TRY(DevBuf::pool(ctx, cb, &pc));
  hipStream_t st = ctx->s_main;
  StreamDrain drain{st};                         // (the caller's arrays are borrowed by the copies)
  LPGP_HIP(hipMemsetAsync(pa.as(), 0, ab, st));
  LPGP_HIP(hipMemsetAsync(pb.as(), 0, bb, st));
  LPGP_HIP(hipMemcpy2DAsync(pa.as(), (size_t)a_ld * sizeof(double), B_host, (size_t)a_src_ld * sizeof(double), (size_t)a_src_ld * sizeof(double),
                            (size_t)a_src_cols, hipMemcpyHostToDevice, st));
  LPGP_HIP(hipMemcpy2DAsync(pb.as(), (size_t)b_ld * sizeof(double), A_host, (size_t)b_src_ld * sizeof(double), (size_t)b_src_ld * sizeof(double),
                            (size_t)b_src_cols, hipMemcpyHostToDevice, st));
  if (beta != 0.0) {
    LPGP_HIP(hipMemsetAsync(pc.as(), 0, cb, st));
    LPGP_HIP(hipMemcpy2DAsync(pc.as(), (size_t)np_ * sizeof(double), C_host, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)m,
                              hipMemcpyHostToDevice, st));
  }
  LPGP_TRY(launch_gemm(ctx, st, transb ? 1 : 0, transa ? 0 : 1,
                       mk(pa.as(), a_ld, pb.as(), b_ld, pc.as(), np_, (int)(np_ / TILE), (int)(mp / TILE), (int)kp, alpha, beta, 0), LPGP_K_GEMM));
  LPGP_HIP(hipMemcpy2DAsync(C_host, (size_t)n * sizeof(double), pc.as(), (size_t)np_ * sizeof(double), (size_t)n * sizeof(double), (size_t)m,
                            hipMemcpyDeviceToHost, st));
  return drain.wait();
}

int lpgp_rhs_to_host(lpgp_ctx* ctx, const lpgp_mat* mat, lpgp_rhs* rhs, double* out_host) {
  LPGP_CHECK(ctx && mat && rhs && out_host, "lpgp_rhs_to_host: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(rhs->ld == mat->pn, "lpgp_rhs_to_host: size mismatch");
  std::vector<double> h((size_t)rhs->ld * rhs->m);
  {
    int rc = rhs_clear_unassembled(ctx, mat, rhs);
    if (rc != 0) return rc;
  }
  LPGP_HIP(hipStreamSynchronize(ctx->s_main));       // assembly launches are asynchronous
  LPGP_HIP(hipMemcpy(h.data(), rhs->v, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> col((size_t)mat->n);
  for (int64_t j = 0; j < rhs->m; ++j) {
    mat->gather_padded(h.data() + j * rhs->ld, col.data());
    for (int64_t i = 0; i < mat->n; ++i) out_host[i * rhs->m + j] = col[(size_t)i];
  }
  return 0;
}

int lpgp_kernel_diag(lpgp_ctx* ctx, const lpgp_kdesc* kd, int32_t ngroups, double* out_value) {
  LPGP_CHECK(kd && out_value, "lpgp_kernel_diag: null argument");
  (void)ctx;
  DevDesc desc;
  int rc = lower_kdesc(kd, ngroups, &desc);
  if (rc != 0) return rc;
  *out_value = desc_diag(desc);      // at x == x' every r_d = 0
  return 0;
}

int lpgp_kernel_matrix(lpgp_ctx* ctx, const lpgp_kdesc* kd, int32_t ngroups, const lpgp_pts* X0,
                       const lpgp_pts* X1, double* out_host) {
  LPGP_CHECK(ctx && kd && X0 && X1 && out_host, "lpgp_kernel_matrix: null argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(X0->d == X1->d && kd[0].d == X0->d, "lpgp_kernel_matrix: dimension mismatch");
  if (X0->n == 0 || X1->n == 0) return 0;
  DevDesc desc;
  LPGP_TRY(lower_kdesc(kd, ngroups, &desc));
  const int64_t ld = round_up(X0->n, 2);
  std::vector<double> h((size_t)ld * X1->n);
  DevBuf d;
  LPGP_TRY(DevBuf::raw(h.size() * sizeof(double), &d));
  StreamDrain drain{ctx->s_main};
  LPGP_TRY(launch_assemble(ctx, ctx->s_main, desc, X0->x, X0->n, X0->n_pad, X1->x, X1->n, X1->n_pad, d.as(), ld, 0, 0, 0));
  LPGP_HIP(hipMemcpyAsync(h.data(), d.as(), h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
  LPGP_TRY(drain.wait());
  for (int64_t i = 0; i < X0->n; ++i)
    for (int64_t j = 0; j < X1->n; ++j) out_host[i * X1->n + j] = h[(size_t)(i + j * ld)];
  return 0;
}

// ---- measurement ----------------------------------------------------------------------------
int lpgp_kernel_matvec(lpgp_ctx* ctx, const lpgp_kdesc* kd, int32_t ngroups, const lpgp_pts* X0,
                       const lpgp_pts* X1, const double* v_host, int64_t nrhs, double* out_host) {
  LPGP_CHECK(ctx && kd && X0 && X1 && v_host && out_host && nrhs >= 1, "lpgp_kernel_matvec: bad argument");
  LPGP_DEVICE(ctx);
  LPGP_CHECK(X0->d == X1->d && kd[0].d == X0->d, "lpgp_kernel_matvec: dimension mismatch");
  const int64_t n0 = X0->n, n1 = X1->n;
  if (n0 == 0) return 0;
  if (n1 == 0) {
    std::memset(out_host, 0, (size_t)(n0 * nrhs) * sizeof(double));
    return 0;
  }
  DevDesc desc;
  LPGP_TRY(lower_kdesc(kd, ngroups, &desc));
  // enough workgroups to fill the chip: row tiles x column splits >= ~4 per CU
  const int tiles_r = (int)((n0 + 63) / 64), tiles_c = (int)((n1 + 63) / 64);
  int splits = (4 * ctx->cus + tiles_r - 1) / tiles_r;
  if (splits > tiles_c) splits = tiles_c;
  if (splits < 1) splits = 1;
  const int64_t n0p = X0->n_pad, n1p = X1->n_pad;
  const size_t bv = (size_t)MV_RHS * n1p * sizeof(double), bp = (size_t)splits * MV_RHS * n0p * sizeof(double),
               bo = (size_t)MV_RHS * n0p * sizeof(double);
  std::vector<double> hv((size_t)MV_RHS * n1p), ho((size_t)MV_RHS * n0p);
  DevBuf buf;
  LPGP_TRY(DevBuf::pool(ctx, bv + bp + bo, &buf));
  double* const dv = buf.as();
  double* const dpart = dv + (size_t)MV_RHS * n1p;
  double* const dout = dpart + (size_t)splits * MV_RHS * n0p;
  for (int64_t r0 = 0; r0 < nrhs; r0 += MV_RHS) {
    const int nr = (int)((nrhs - r0 < MV_RHS) ? nrhs - r0 : MV_RHS);
    for (int r = 0; r < nr; ++r)
      for (int64_t j = 0; j < n1; ++j) hv[(size_t)r * n1p + j] = v_host[j * nrhs + r0 + r];
    StreamDrain drain{ctx->s_main};              // (the staging vectors are borrowed by the copies of this pass)
    LPGP_HIP(hipMemcpyAsync(dv, hv.data(), (size_t)nr * n1p * sizeof(double), hipMemcpyHostToDevice, ctx->s_main));
    LPGP_TRY(launch_matvec(ctx, ctx->s_main, desc, X0->x, n0, n0p, X1->x, n1, n1p, dv, nr, dpart, splits, dout));
    LPGP_HIP(hipMemcpyAsync(ho.data(), dout, (size_t)nr * n0p * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
    LPGP_TRY(drain.wait());
    for (int r = 0; r < nr; ++r)
      for (int64_t i = 0; i < n0; ++i) out_host[i * nrhs + r0 + r] = ho[(size_t)r * n0p + i];
  }
  return 0;
}

int lpgp_profile_enable(lpgp_ctx* ctx, int32_t mask) {
  LPGP_DEVICE(ctx);
  int rc = prof_collect(ctx);
  ctx->prof_on = mask;
  return rc;
}

int lpgp_profile_reset(lpgp_ctx* ctx) {
  LPGP_DEVICE(ctx);
  int rc = prof_collect(ctx);
  for (auto& s : ctx->prof) s = ProfSlot();
  return rc;
}

int lpgp_profile_get(lpgp_ctx* ctx, int32_t kernel_id, double* ms, int64_t* launches, double* flops, double* bytes) {
  LPGP_CHECK(kernel_id >= 0 && kernel_id < LPGP_K_COUNT, "lpgp_profile_get: bad kernel id");
  LPGP_DEVICE(ctx);
  int rc = prof_collect(ctx);
  if (rc != 0) return rc;
  const ProfSlot& s = ctx->prof[kernel_id];
  if (ms) *ms = s.ms;
  if (launches) *launches = s.launches;
  if (flops) *flops = s.flops;
  if (bytes) *bytes = s.bytes;
  return 0;
}

}  // extern "C"
