// Internal declarations shared by the HIP translation units of liblpgp.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "lpgp.h"
#include "lpgp_desc.h"
#include "factor_view.h"
#include "mat_state.h"
#include "pivchol_state.h"
#include "options.h"

namespace lpgp {

// ---- 2-D block-cyclic distribution ------------------------------------------------------
// Tiles of 128 are dealt in blocks of nbt tiles (nb = 512 columns): global tile g belongs to block g / nbt, owned by
// member (g / nbt) % P of its process row / column.  A member stores its tiles in increasing global order.
struct Cyc {
  int32_t P = 1, me = 0, nbt = 4;
};
__host__ __device__ inline int cyc_owner(const Cyc& c, int g) { return (g / c.nbt) % c.P; }
// number of tiles with global index < g that `me` owns == local index of global tile g if owned
__host__ __device__ inline int cyc_before(const Cyc& c, int g) {
  const int B = g / c.nbt, rem = g - B * c.nbt;
  return ((B + c.P - 1 - c.me) / c.P) * c.nbt + ((B % c.P) == c.me ? rem : 0);
}
__host__ __device__ inline int cyc_l2g(const Cyc& c, int l) {
  const int lb = l / c.nbt;
  return (lb * c.P + c.me) * c.nbt + (l - lb * c.nbt);
}
// global padded index -> local index, or -1 if another member owns it
__host__ __device__ inline int64_t cyc_local(const Cyc& c, int64_t gi) {
  if (c.P == 1) return gi;                       // single member: local == global (no divisions on the single-GPU path)
  const int g = (int)(gi / TILE);
  if (cyc_owner(c, g) != c.me) return -1;
  return (int64_t)cyc_before(c, g) * TILE + (gi - (int64_t)g * TILE);
}
// where a rank keeps element (row, column) of the global padded matrix: (row cyclic over Pr, column over Pc)
struct Layout2D {
  Cyc rows, cols;
};



#define LPGP_HIP(expr)                                                              \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      ::lpgp::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr,                \
                        hipGetErrorString(_e));                                     \
      return -1;                                                                    \
    }                                                                               \
  } while (0)

#define LPGP_TRY_RC(expr)         \
  do {                            \
    int _rc = (expr);             \
    if (_rc != 0) return _rc;     \
  } while (0)
#define LPGP_TRY(expr) LPGP_TRY_RC(expr)

// ---- profiling -------------------------------------------------------------------------
struct ProfSlot {
  double ms = 0.0;
  int64_t launches = 0;
  double flops = 0.0;
  double bytes = 0.0;
};

struct PendingEvent {
  hipEvent_t e0, e1;
  int kernel;
};

}  // namespace lpgp

struct lpgp_ctx : lpgp::Options {     // tuning options: options.h
  int device = 0;
  int cus = 0;
  hipStream_t s_main = nullptr;    // panel / critical-path stream (high priority)
  hipStream_t s_upd = nullptr;     // trailing-update stream (all CUs but `reserve_cus`)
  hipStream_t s_upd_narrow = nullptr;  // same with `reserve_narrow` CUs (default 64) left to the panel chain
  hipStream_t s_upd_all = nullptr;     // unmasked update stream: the blocked solves have no whole-CU kernel to protect
  hipStream_t s_outer = nullptr;       // rank-nb_outer updates (a1), (b) of the factorisation (masked like s_upd)
  hipEvent_t ev_outer[2] = {nullptr, nullptr};
  hipEvent_t ev_outer_fact[2] = {nullptr, nullptr};
  hipEvent_t ev_outer_a1[2] = {nullptr, nullptr};
  hipEvent_t ev_chain_pre = nullptr;   // recorded on the panel stream right in front of a resident chain launch: a kernel that follows the chain through
                                       // its flags (panel_chain_v_kernel) is not dispatched before the chain kernel itself can be
  hipEvent_t ev_ride[4] = {nullptr, nullptr, nullptr, nullptr};   // ride-along substitution (potrf_predict_blocked): panel hand-overs [0, 1], fork / join [2, 3]
  hipEvent_t ev_append[2] = {nullptr, nullptr};
  hipEvent_t ev_chain_rows = nullptr;
  int* d_chain_flags = nullptr;        // ring of flag slots (zeroed; a launch zeroes the slot half a ring ahead)
  int64_t chain_launches = 0;          // resident chain launches so far: launch n takes slot n % ring (its followers get the slot by ChainTicket)
  // Route counters (read-only through lpgp_get_option, keys "route_*"): incremented on the host where a forward substitution
  // picks its branch, for the tests that must prove which branch they ran (the profiling slots cannot tell these apart).
  struct RouteCounts {
    int64_t ride_done = 0;             // potrf_predict_blocked: nothing left to factor, the plain substitution
    int64_t ride_aug = 0;              // ... the augmented form
    int64_t ride_b2b = 0;              // ... factorisation and substitution back to back (ride_max_tiles)
    int64_t ride = 0;                  // ... the substitution riding inside the factorisation
    int64_t ride_vchain = 0;           // ride panel steps that followed the resident chain (panel_chain_v_kernel)
    int64_t ride_two = 0;              // ride panel steps split into two halves on two streams
    int64_t ride_outer = 0;            // ride outer blocks closed by their one outer update (two-level ride; once, not per half)
    int64_t solve_two_level = 0;       // trsm_lower_blocked: the two-level form
    int64_t solve_ahead = 0;           // ... fused look-ahead launches (panel_solve_kernel with the update in front)
    int64_t solve_tiles = 0;           // ... panels solved tile by tile (not fused)
  } route;
  hipEvent_t ev_panel[2] = {nullptr, nullptr};
  hipEvent_t ev_upd[2] = {nullptr, nullptr};
  // lpgp_mat_inverse_diag / lpgp_mat_loo (evidence.hip): columns of the identity solved at a time (a multiple of 128, at most 4 096: the
  // right-hand side takes 8 n x this many bytes), and the bytes these entry points and lpgp_mat_evidence have copied up and down --
  // option "inverse_diag_panel" and the read-only keys "evidence_h2d_bytes" / "evidence_d2h_bytes" of lpgp_get_option
  int64_t inverse_diag_panel = 4096;
  int64_t cv_fold_batch = 512;     // lpgp_mat_cv (evidence_cv.hip): folds of at most 128 rows per launch, 256 KiB of scratch each -- option "cv_fold_batch"
  int64_t evidence_h2d_bytes = 0, evidence_d2h_bytes = 0;
  // workspace
  // descriptor ring: an assembly launch copies its lowered descriptor into a pinned host slot,
  // from there (truly asynchronously) into the slot's device copy; the slot is reused only
  // after the event recorded behind its kernel has fired -- no stream sync per assembly call
  static constexpr int DESC_RING = 8;
  struct DescSlot { lpgp::DevDesc* h = nullptr; lpgp::DevDesc* d = nullptr; hipEvent_t done = nullptr; bool used = false; };
  DescSlot desc_ring[DESC_RING];
  int desc_next = 0;
  int* d_info = nullptr;           // potrf info word
  int* h_info_pinned = nullptr;    // pinned mirror, 16 ints (multi-GPU: a device-to-host copy into pageable memory would BLOCK behind a collective that waits for a dead peer)
  enum PinnedSlot {                // one slot of h_info_pinned per reader, so that no two of them share a word
    PIN_ALLREDUCE = 0,             // allreduce_max_int (dist.hip): the value on its way to the device and back
    PIN_POTRF_DIST = 1,            // potrf_dist: this rank's own status, before the ranks agree on one
    PIN_POTRF_PREDICT = 4,         // lpgp_potrf_predict: the matrix's sticky word, read back with the prediction's results
    PIN_POTRF = 5,                 // potrf_blocked_impl: the status of a factorisation that reports to the caller (lpgp_potrf)
    PIN_SOLVE_WEIGHTS = 6,         // lpgp_solve_weights: the status of the single-vector solve
  };
  double* d_tmp = nullptr;         // small scratch (vectors)
  int64_t tmp_cap = 0;
  double* h_stage = nullptr;       // pinned host staging for the results of a prediction: ONE asynchronous device-to-host copy and
  double* h_stage_r = nullptr;     // ... and for the residual on its way up (lpgp_mat_set_residual: no wait at all)
  int64_t stage_r_cap = 0;
  hipEvent_t ev_stage_r = nullptr;
  int64_t stage_cap = 0;           // one wait per call (a copy into pageable memory is a blocking round trip of its own, ~25 us each)
  // caching allocator: freed device buffers are kept for reuse (a hipMalloc/hipFree pair
  // of a multi-GB Gram matrix costs more than the factorisation of a small problem)
  struct PoolBuf { void* p; size_t bytes; };
  std::vector<PoolBuf> pool;
  // Test hook (lpgp_test_pool_fill; never set by the product): >= 0: every buffer pool_alloc or ensure_tmp hands out is first
  // filled with this byte, on the panel stream, so that a read of storage nobody wrote shows in the results
  int pool_fill = -1;
  int64_t pool_filled[2] = {0, 0};   // buffers and bytes filled since the hook last asked
  // Point sets handed over per call (the reference's calling convention: NumPy arrays) come and go with every step of a small
  // problem: their device buffers are recycled here (hipMalloc + hipFree cost ~50 us a pair, and hipFree waits for the device),
  // their uploads go through a ring of pinned slots on the panel stream -- where every kernel that reads a point set runs --
  // without a wait (lpgp_pts_create / lpgp_pts_destroy; single GPU)
  std::vector<PoolBuf> pts_pool;
  static constexpr int PTS_SLOTS = 8;
  static constexpr size_t PTS_SLOT_BYTES = 64 << 10;
  struct PtsSlot { void* h = nullptr; hipEvent_t done = nullptr; bool used = false; };
  PtsSlot pts_ring[PTS_SLOTS];
  int pts_next = 0;
  // multi-GPU (one process per GPU): Pr x Pc process grid, rank = r * Pc + c; 2-D block-cyclic tiles
  int rank = 0, world = 1;
  int pr = 1, pc = 1;
  int grid_set = 0;                // lpgp_dist_set_grid called (else a default grid is chosen at init)
  int dist_broken = 0;             // the communicator was aborted after a failure inside a collective call
  int live_mats = 0;               // matrices / right-hand sides alive: their storage was laid out for the CURRENT grid (lpgp_dist_set_grid)
  double comm_bytes_sent = 0.0, comm_bytes_recv = 0.0;
  hipStream_t s_comm = nullptr;    // panel exchange (RCCL point-to-point group calls)
  hipEvent_t ev_comm[2] = {nullptr, nullptr};
  void* nccl_comm = nullptr;       // ncclComm_t
  void* nccl_comm_bulk = nullptr;  // second communicator (ncclCommSplit of the first): the bulk of a split panel gather travels on it,
                                   // beside the small exchanges of the panel chain (operations on ONE communicator are serialised)
  hipEvent_t ev_tail[2] = {nullptr, nullptr};   // the bulk part of the gather into panel buffer 0 / 1 has landed
  hipEvent_t ev_rows[2] = {nullptr, nullptr};   // the rows below panel i are solved (the bulk gather may read them)
  double* d_pack_bulk = nullptr;   // pack / receive buffer of the bulk part
  size_t pack_bulk_cap = 0;
  lpgp_host_exchange_fn host_xfer = nullptr;   // test transport (lpgp_dist_init_host): panels staged through the host
  void* host_xfer_user = nullptr;
  // direct-peer transport (lpgp_dist_init_ipc): every rank owns a receive window in HBM, mapped into every peer by
  // IPC handle; a root pushes its pieces straight into the peers' windows (device-to-device copies over xGMI / inside
  // the GPU), the host exchange above only carries the barriers between the phases of an exchange
  double* ipc_window = nullptr;               // this rank's window
  size_t ipc_window_doubles = 0;              // used as two halves: [0]: exchanges of the panel stream, [1]: bulk exchanges of the exchange stream
  hipEvent_t ev_ipc[2] = {nullptr, nullptr};  // completion of the last copy-out of each half (the half may be pushed into again after it)
  int ipc_copyout_pending[2] = {0, 0};
  std::vector<double*> ipc_peer;              // window of rank r as mapped here (own window for r == rank)
  bool ipc() const { return !ipc_peer.empty(); }
  bool distributed() const { return nccl_comm != nullptr || host_xfer != nullptr || dist_broken; }
  double* d_pack = nullptr;        // packed panel pieces: [own piece | pieces received from the other sources]
  size_t pack_cap = 0;             // doubles
  double* d_panel[2] = {nullptr, nullptr};   // gathered panel, dense, global row order (double-buffered for the look-ahead)
  size_t panel_cap[2] = {0, 0};    // doubles
  lpgp::Layout2D layout() const {
    lpgp::Layout2D l;
    l.rows.P = pr; l.rows.me = rank / pc; l.rows.nbt = (int32_t)(nb / lpgp::TILE);
    l.cols.P = pc; l.cols.me = rank % pc; l.cols.nbt = (int32_t)(nb / lpgp::TILE);
    return l;
  }
  // kernels whose dynamic-LDS attribute has been raised on THIS context's device (the attribute is
  // per device, a process-wide flag would skip it for a second context on another GPU)
  std::vector<const void*> lds_attr_done;
  // profiling
  int prof_on = 0;                 // bit k: bracket launches of kernel id k with HIP events
  int prof_open = 0;
  lpgp::ProfSlot prof[LPGP_K_COUNT];
  std::vector<lpgp::PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;
};

struct lpgp_pts {
  lpgp_ctx* ctx;
  int64_t n;
  int32_t d;
  double* x;                       // device, SoA: x[dim * n_pad + i]
  int64_t n_pad;
  size_t bytes = 0;                // size of the allocation behind x
};

// The stencil table of one block of matrix observations (mix_table.h), resident: ONE allocation, weights first.
struct lpgp_mix {
  lpgp_ctx* ctx;
  int64_t q;                       // rows of the block
  int32_t S;                       // row width, 1 .. LPGP_MAXS
  int64_t npts;                    // size of the point set the indices were checked against
  double* w;                       // device, slot-major: w[s * q + r]
  int32_t* idx;                    // device, behind w: idx[s * q + r]
};

struct lpgp_mat : lpgp::MatState {  // block table and factor state: mat_state.h
  lpgp_ctx* ctx = nullptr;
  int64_t cap = 0;                 // padded capacity of the GLOBAL matrix (multiple of TILE); single GPU: == leading dimension
  int64_t lr_cap = 0, lc_cap = 0;  // rows / columns of this rank's share (== cap on a single GPU); lr_cap is the leading dimension of a
  double* dblk = nullptr;          // multi-GPU only: the nb x nb diagonal blocks of the factor, replicated on every rank:
                                   //   block K at dblk + K * nb * nb, column-major, leading dimension nb
  double* a = nullptr;             // device lr_cap x lc_cap column-major (lower part meaningful): this rank's tiles
  double* linv = nullptr;          // device (cap/TILE) tiles of TILE x TILE: inverse of each diagonal tile of L
  double* w = nullptr;             // device 2*cap: [representer weights | residual r] (padded layout)
  int* d_status = nullptr;         // device word: first non-positive pivot of the factorisations enqueued since the last lpgp_mat_check (sticky)
  double* r() const { return w + cap; }
};
static_assert(lpgp::MatState::TB == lpgp::TILE, "the tile edge");

struct lpgp_rhs {
  lpgp_ctx* ctx;
  int64_t ld;                      // padded row capacity (multiple of TILE)
  int64_t m;                       // columns
  int64_t m_pad;                   // multiple of TILE, > m: column m is spare (carries the residual through the solve)
  double* v;                       // device ld x m_pad column-major
  std::vector<char> assembled;     // per observation block: rows written by lpgp_cross_assemble (the others are cleared on first use)
};

// A pivoted Cholesky G ~ L^T L of a Gram OPERATOR, resident (pivchol.hip).  The loop state and the column coverage of the pending row
// are PivcholState's (pivchol_state.h); the buffers below are written by the kernels of pivchol.hip only.  An lpgp_pcg created by
// lpgp_pcg_create_pivchol reads L in place (pcg.hip).
struct lpgp_pivchol : lpgp::PivcholState {
  lpgp_ctx* ctx = nullptr;
  double* L = nullptr;             // device max_rank x n, row-major: the layout pcg_lr_kernel / pcg_z_kernel read
  size_t L_bytes = 0;
  double* work = nullptr;          // device: d[n] | row[2 n] | one point[LPGP_MAXD * 64] | partials[3 * 256] | slot[4]
  size_t work_bytes = 0;
  double* d() const { return work; }
  double* row() const { return work + n; }       // entry j at row()[2 j]: the leading dimension lpgp_kernel_matrix gives one point
  double* one() const { return work + 3 * n; }   // a one-point set, padded to 64 as lpgp_pts_create pads it
  double* part() const { return one() + LPGP_MAXD * 64; }
  double* slot() const { return part() + 3 * 256; }   // {pivot (int64; -2: a NaN in d), d[pivot], sum of d}
};

namespace lpgp {

// every C-ABI entry point runs on its context's device whatever the calling thread's current device is
// (a negative status used to be reported ONCE -- lpgp_mat_check cleared `unchecked` first -- and the next prediction ran on a garbage factor)
#define LPGP_MAT_ALIVE(mat, fn) \
  LPGP_CHECK(!(mat)->poisoned, fn ": the factor of this matrix is undefined (an earlier factorisation timed out or failed half way); condition again from the prior")

#define LPGP_DEVICE(ctx)                                        \
  do {                                                          \
    LPGP_CHECK((ctx) != nullptr, "null context handle");        \
    LPGP_HIP(hipSetDevice((ctx)->device));                      \
  } while (0)

// a transition of mat_state.h that refused (rc != 0): its text becomes the error
inline int refused(int rc, const std::string& err) {
  if (rc != 0) set_error("%s", err.c_str());
  return rc;
}

// The factor of a single-GPU matrix as the drivers of potrf.hip, chain.hip and trsv.hip take it.  The leading dimension is that of
// this rank's share, lr_cap; the drivers address GLOBAL tiles with it, which is right only where the share is the whole matrix:
// this is the one place that says so.
inline int factor_view(const lpgp_mat* mat, FactorView* out) {
  LPGP_CHECK(mat->lr_cap == mat->cap, "single-GPU driver on a distributed matrix: leading dimension %lld, capacity %lld", (long long)mat->lr_cap,
             (long long)mat->cap);
  *out = FactorView{mat->a, mat->linv, mat->lr_cap};
  return 0;
}

// raise the dynamic shared-memory limit of `fn` once per context (= per device)
inline int ensure_lds_attr(lpgp_ctx* ctx, const void* fn, size_t bytes) {
  for (const void* f : ctx->lds_attr_done)
    if (f == fn) return 0;
  LPGP_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  ctx->lds_attr_done.push_back(fn);
  return 0;
}

// Wait for `stream` (dist.hip).  With an RCCL communicator of more than one rank this is NOT hipStreamSynchronize: a peer
// that failed has aborted its communicator, and a kernel of this rank that still waits for that peer's data would wait for
// ever.  The stream is polled instead, RCCL's asynchronous error state is checked every few milliseconds, and on a remote
// error -- or after LPGP_DIST_TIMEOUT_S seconds (default 600, 0: none) -- this rank aborts its own communicator, which
// terminates the pending kernels, and returns an error (the context is unusable afterwards, `dist_broken`).
int sync_stream(lpgp_ctx* ctx, hipStream_t stream);
// One tiny message between every pair of ranks and one all-reduce, checked (dist.hip; called by lpgp_dist_init while every
// rank is known to be alive): RCCL sets its connections up at first use, inside a BLOCKING host call -- later, with a peer
// gone, that call would never return; after this every exchange only enqueues kernels, which sync_stream can watch.
int dist_warm_up(lpgp_ctx* ctx);
// Link probe (dist.hip; lpgp_dist_link_probe): measured unidirectional rate of every ordered pair of ranks, of one rank
// sending to all others at once and of all ranks doing so at once, through the transport the panel exchanges use.
int dist_link_probe(lpgp_ctx* ctx, int64_t bytes, int32_t reps, double* out);

// device memory pool (api.hip)
int pool_alloc(lpgp_ctx* ctx, void** out, size_t bytes, bool* fresh);
void pool_free(lpgp_ctx* ctx, void* p, size_t bytes);

// ---- scope guards of the entry points: the error macros return early, these release on the way out -------------------------
#define LPGP_LOCAL __attribute__((visibility("hidden")))      // (their inline members are no exports of the library)
// A temporary device buffer.  It goes back where it came from when it leaves its scope: into the pool (reuse of a pool buffer is
// ordered on the panel stream, so the guard may go right after the last launch that uses the buffer was enqueued there), or to
// hipFree (which waits for the device).
class LPGP_LOCAL DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p_ && ctx_) pool_free(ctx_, p_, bytes_);
    else if (p_) (void)hipFree(p_);
  }
  static int pool(lpgp_ctx* ctx, size_t bytes, DevBuf* out) {
    LPGP_TRY(pool_alloc(ctx, &out->p_, bytes, nullptr));
    out->ctx_ = ctx;
    out->bytes_ = bytes;
    return 0;
  }
  static int raw(size_t bytes, DevBuf* out) {
    const hipError_t e = hipMalloc(&out->p_, bytes);
    if (e != hipSuccess) {
      out->p_ = nullptr;
      set_error("device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
      return -1;
    }
    return 0;
  }
  void adopt_raw(void* p) { p_ = p; }      // a pointer that came from hipMalloc earlier (the points-set recycler)
  template <class T = double> T* as() const { return static_cast<T*>(p_); }
  void* release() {                        // hand the pointer to a longer-lived owner (lpgp_rhs::v, lpgp_dvec::v, ...)
    void* p = p_;
    p_ = nullptr;
    return p;
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
  lpgp_ctx* ctx_ = nullptr;                // pool buffers only
};

// Borrowed host memory is drained before return: a function that enqueues a copy to or from a local vector or the caller's
// pointer declares one of these BEHIND the vector and the device buffers, waits through wait() on its way to success, and is
// waited for by the destructor on every early return (which keeps the error text of the step that failed).
// `watched`: the context of a multi-GPU path, whose waits go through sync_stream.
struct LPGP_LOCAL StreamDrain {
  hipStream_t st;
  lpgp_ctx* watched = nullptr;
  bool armed = true;
  int wait() {
    armed = false;
    if (watched) return sync_stream(watched, st);
    LPGP_HIP(hipStreamSynchronize(st));
    return 0;
  }
  ~StreamDrain() {
    if (!armed) return;
    const std::string msg = last_error();
    if (wait() != 0) set_error("%s", msg.c_str());
  }
};

// two timing events (micro-benchmarks of the test hooks, the link probe)
struct LPGP_LOCAL EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int create() {
    LPGP_HIP(hipEventCreate(&e0));
    LPGP_HIP(hipEventCreate(&e1));
    return 0;
  }
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// profiling helpers: bracket launches of `kernel` on `stream`
void prof_begin(lpgp_ctx* ctx, hipStream_t stream, int kernel, double flops, double bytes);
void prof_end(lpgp_ctx* ctx, hipStream_t stream);
// ... paired on every way out of the scope of the launch
struct LPGP_LOCAL ProfScope {
  lpgp_ctx* ctx;
  hipStream_t stream;
  ProfScope(lpgp_ctx* c, hipStream_t s, int kernel, double flops, double bytes) : ctx(c), stream(s) { prof_begin(c, s, kernel, flops, bytes); }
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
  ~ProfScope() { prof_end(ctx, stream); }
};
int prof_collect(lpgp_ctx* ctx);

// gemm.hip --------------------------------------------------------------------------------
// C(m x n) = beta*C + alpha*A*B.  All of m, n multiples of TILE, k multiple of 16.
// ta: A element (i,kk) at A[i + kk*lda] (0) or A[kk + i*lda] (1);
// tb: B element (kk,j) at B[j + kk*ldb] (0) or B[kk + j*ldb] (1).
// tri: 0 full; 1 / 2 / 3 lower-only (C(0,0) is a diagonal tile): tiles with row tile < column
//      tile are skipped (1: rank-nb trailing update, remainder
//      half; 3: its look-ahead half; 2: rank-128 update inside a panel -- same code, own kernel
//      symbol and profiling slot each).
struct GemmArgs {
  const double* A;
  const double* B;
  double* C;
  int64_t lda, ldb, ldc;
  int32_t mt, nt;                  // tiles in m and n
  int32_t k;
  double alpha, beta;
  int32_t tri;
  int32_t occ3 = 1;                // the launch may use the three-workgroups-per-CU kernel (the schedulers clear it while the panel chain runs beside the update: see factor_columns)
  int32_t sshift = 3;              // log2 of the super-tile edge (set by launch_gemm; legacy mapping)
  // dense tile enumeration (set by launch_gemm; map_tile_dense in gemm.hip)
  int32_t dense = 0;
  int32_t ntiles = 0, chunk = 0, nbands = 0, band = 8;
  static constexpr int MAXB = 192; // bands of 8 tile rows: 1536 tile rows = 196 608 matrix rows (> 288 GB of fp64)
  int32_t band_prefix[MAXB + 1];   // triangular shapes only: tiles before band b
  // distributed trailing update (cyc != 0, triangular shapes, dense enumeration): C is a region of this rank's
  // LOCAL tiles -- local tile row tr / column tc stand for the global tiles gr = cyc_l2g(rowc, rt0 + tr) and
  // gc = cyc_l2g(colc, ct0 + tc) -- and both operands are rows of ONE dense panel in global row order that
  // starts at global tile g0: A tile = A + (gr - g0) * 128, B tile = B + (gc - g0) * 128.  A tile is valid iff
  // gr >= gc: a staircase, enumerated band by band like the triangle (map_tile_stair in gemm.hip).
  int32_t cyc = 0;
  Cyc rowc, colc;
  int32_t rt0 = 0, ct0 = 0, g0 = 0;
  unsigned long long* stamps = nullptr;   // diagnostic builds (-DLPGP_STAMP) only
  unsigned long long* timeline = nullptr; // diagnostic builds: per-workgroup life cycle + hardware id
};
inline GemmArgs mk(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int mt, int nt, int k, double alpha,
                   double beta, int tri) {
  GemmArgs g;
  g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.mt = mt; g.nt = nt; g.k = k; g.alpha = alpha; g.beta = beta;
  g.tri = tri;
  return g;
}
int launch_gemm(lpgp_ctx* ctx, hipStream_t stream, int ta, int tb, const GemmArgs& g, int prof_kernel);
int stair_enumerate_host(const GemmArgs& g, int32_t* out, int64_t cap);
int64_t gemm_valid_tiles(const GemmArgs& g);
// dist.hip: the arguments of the distributed trailing update of one rank (potrf_dist; the test hook lpgp_test_gemm_cyc): local tile
// rows [rt0, rt1) x local tile columns [ct0, ct1) of the storage `a` (leading dimension ld) of the member R x C of the grid, updated by
// the gathered panel (first global tile row g0, leading dimension ldp, K128 columns): alpha = -1, beta = 1
GemmArgs update_args(double* a, int64_t ld, const Cyc& R, const Cyc& C, const double* panel, int64_t ldp, int g0, int K128, int rt0, int rt1,
                     int ct0, int ct1, int tri);
// Tile solves with one step of iterative refinement (solve.hip: tile_solve_kernel); L = the 128 x 128 diagonal
// tile of the factor (leading dimension ldl, zeros above the diagonal), linv its explicit inverse (ld 128):
// X (mt*128 rows x 128, column-major ldx) <- X L^{-T} in place
// V (128 rows x nt*128 columns, column-major ldv) <- L^{-1} V in place (tile step of the forward substitution)
int launch_trsv_tile(lpgp_ctx* ctx, hipStream_t stream, double* V, int64_t ldv, const double* linv, const double* L, int64_t ldl,
                     int nt, int prof_kernel);
int launch_trsm_tile(lpgp_ctx* ctx, hipStream_t stream, double* X, int64_t ldx, const double* linv, const double* L, int64_t ldl,
                     int mt, int prof_kernel);
// the whole chain of a panel of the forward substitution in one launch (solve_panel.h: panel_solve_kernel): V (nt_rows <= 4
// tiles of rows, top row at V) <- L_KK^{-1} V; linv: the panel's tile inverses (contiguous), L: its diagonal block.
// lds_extra: bytes of LDS the launch asks for beyond the kernel's own 69 632, at most PANEL_LDS_PAD (solve_panel.h: launch_panel_solve_rg)
constexpr int PANEL_LDS_PAD = 20480;
int launch_trsv_panel(lpgp_ctx* ctx, hipStream_t stream, double* V, int64_t ldv, const double* linv, const double* L, int64_t ldl,
                      int nt_rows, int nt_cols, int prof_kernel, int lds_extra = 0);
// the same chain for rows: X (mt tiles of rows x nt_cols <= 4 tile columns) <- X L_KK^{-T}, L_KK already factored
// the same with the look-ahead update by the previous panel (4 tiles = 512 solved rows right above V) fused in front (solve4p.hip)
int launch_trsv_panel_ahead(lpgp_ctx* ctx, hipStream_t stream, double* V, int64_t ldv, const double* linv, const double* L, const double* Lprev,
                            int64_t ldl, int nt_rows, int nt_cols, int prof_kernel);
int launch_trsm_panel(lpgp_ctx* ctx, hipStream_t stream, double* X, int64_t ldx, const double* linv, const double* L, int64_t ldl,
                      int nt_cols, int mt, int prof_kernel);

// chain.hip: the whole chain of panel [p0, p0 + 4) (rows down to tile T) in one launch.  *ticket: what a launch that follows this
// chain through its flags is given (launch_panel_chain_rows, launch_panel_chain_v); it names ONE chain launch, whatever is launched after it
struct ChainTicket {
  int* slot = nullptr;             // the launch's flag slot in lpgp_ctx::d_chain_flags
  int p0 = -1;                     // its panel
  int64_t seq = -1;                // lpgp_ctx::chain_launches when the slot was taken (the slot is recycled 32 launches later)
};
int launch_panel_chain(lpgp_ctx* ctx, hipStream_t stream, FactorView F, int p0, int T, int* d_info, ChainTicket* ticket, bool rows_here = true, bool ahead = false);
int launch_panel_chain_rows(lpgp_ctx* ctx, hipStream_t stream, FactorView F, const ChainTicket& chain, int p0, int T, int* d_info);
int launch_panel_chain_v(lpgp_ctx* ctx, hipStream_t stream, FactorView F, const ChainTicket& chain, int p0, double* V, int64_t ldv, int64_t cols, int* d_info);
// potrf.hip -------------------------------------------------------------------------------
int debug_tile_xcc(int32_t* out8, int reset);
// The form of a factorisation's tile Cholesky.  newton: the Newton sign in the last correction of a pivot's reciprocal square root
// (potrf_tile.h), for factors whose results are read off the inverse (lpgp_mat_cv's large folds).  The resident panel chain has no
// such form: a factorisation of this form runs without it, every diagonal tile through launch_potrf_tile.
enum class TileForm : int { plain, newton };
int launch_potrf_tile(lpgp_ctx* ctx, hipStream_t stream, double* a, int64_t lda, double* linv,
                      int* d_info, int info_base, TileForm form);
int potrf_blocked(lpgp_ctx* ctx, lpgp_mat* mat, int64_t t_done, int64_t T, int32_t* info, TileForm form = TileForm::plain);
// api.hip: lpgp_potrf in a given form (checks, distributed or single GPU, the matrix's state transitions)
int potrf_mat(lpgp_ctx* ctx, lpgp_mat* mat, int32_t* info, TileForm form);
int potrf_predict_blocked(lpgp_ctx* ctx, lpgp_mat* mat, int64_t t_done, int64_t T, double* v, int64_t ldv, int64_t m_pad);
// dist.hip: Pr x Pc block-cyclic factorisation and panel-streaming solves
int potrf_dist(lpgp_ctx* ctx, lpgp_mat* mat, int64_t t_done, int64_t T, int32_t* info);
int trsm_lower_dist(lpgp_ctx* ctx, lpgp_mat* mat, int64_t T, double* v, int64_t ldv, int64_t m_pad);
int trsm_lower_t_dist(lpgp_ctx* ctx, lpgp_mat* mat, int64_t T, double* v, int64_t ldv, int64_t m_pad);
int factor_to_host_dist(lpgp_ctx* ctx, lpgp_mat* mat, double* out_padded /* pn x pn column-major */);
int copy2d(hipStream_t st, double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t cols);
// (the drivers below work on the factor through a FactorView: the trailing sub-factor L[t0:, t0:] is F.trailing(t0))
int trsm_lower_blocked(lpgp_ctx* ctx, FactorView F, int64_t T, double* v, int64_t ldv, int64_t m_pad);
int trsm_lower_t_blocked(lpgp_ctx* ctx, FactorView F, int64_t T, double* v, int64_t ldv, int64_t m_pad);
// v <- G^{-1} v; tmp: T * 128 + 2 doubles of scratch; info: device status word (INT_MIN after a timed-out hand-over of the resident form)
int solve_vec(lpgp_ctx* ctx, FactorView F, int64_t T, double* v, double* tmp, int* info);
int solve_vec_resident(lpgp_ctx* ctx, FactorView F, int64_t T, double* v, double* tmp, int* info);      // trsv.hip
int solve_vec_fwd(lpgp_ctx* ctx, hipStream_t st, FactorView F, int64_t T, double* b, double* x);
int solve_vec_fwd_resident(lpgp_ctx* ctx, FactorView F, int64_t T, const double* b, double* x, int* info);   // trsv.hip: the forward half alone
// the backward half alone, x <- L^{-T} y.  Per tile row (potrf.hip): y is consumed as the running right-hand side.  Resident (trsv.hip):
// the entries of y are read only; y has T * 128 + 2 doubles, of which the LAST (y + T * 128 + 1) is the ticket word, at -1 (all bits set) on entry
int solve_vec_bwd(lpgp_ctx* ctx, hipStream_t st, FactorView F, int64_t T, double* y, double* x);
int solve_vec_bwd_resident(lpgp_ctx* ctx, FactorView F, int64_t T, double* y, double* x, int* info);
// evidence.hip: the quantities read off the factor of a fully factored single-GPU matrix (lpgp_mat_evidence, lpgp_mat_inverse_diag, lpgp_mat_loo)
// (max_wgs > 0, from the test hooks only: a cap on the workgroups of the stage-1 reduction, so that a thread takes several rows)
int mat_evidence(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, double out_host[2], int max_wgs = 0);
int mat_inverse_diag(lpgp_ctx* ctx, lpgp_mat* mat, double* out_host);
int mat_loo(lpgp_ctx* ctx, lpgp_mat* mat, const double* r_host, const double* y_host, double* mean_host, double* var_host, double* logp_host,
            int max_wgs = 0);
// ... and their pieces that evidence_cv.hip shares: the host staging of nvec logical vectors into the padded layout (behind them the map
// padded row -> logical row as pn int32), the counted copies, diag(G^{-1}) into a device vector of pn doubles
void ev_stage(const lpgp_mat* mat, const double* const* vecs, int nvec, std::vector<double>* h);
int ev_upload(lpgp_ctx* ctx, double* dst, const std::vector<double>& h);
int ev_download(lpgp_ctx* ctx, double* dst, const double* src, size_t doubles);
int inverse_diag_device(lpgp_ctx* ctx, lpgp_mat* mat, double* d_diag);
// evidence_cv.hip: leave-fold-out cross-validation from the dense inverse (lpgp_mat_cv)
int mat_cv(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, const double* r_host, const double* y_host, const int32_t* fold_of, int32_t nfolds,
           double* mean_host, double* var_host, double* logp_host, double* cov_host);
// evidence_grad.hip: the dense inverse W^T W, W = L^{-1}, into the lower triangle of `out` (same block layout, not factored), and the
// pair (w^T dG w, tr(G^{-1} dG)) of GPML eq. 5.9 for an assembled dG / for dG = diag(v) + scalar I on block bi
int mat_inverse_into(lpgp_ctx* ctx, lpgp_mat* mat, lpgp_mat* out);
// what lpgp_mat_evidence_grad, its _diag form and lpgp_mat_cv ask of `other` (the dense inverse, an assembled derivative; `what` names it)
int evidence_grad_layout(const lpgp_mat* mat, const lpgp_mat* other, const char* fn, const char* what);
int mat_evidence_grad(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, const lpgp_mat* dG, const double* r_host, double out_host[2],
                      int max_wgs = 0);
int mat_evidence_grad_diag(lpgp_ctx* ctx, lpgp_mat* mat, const lpgp_mat* ginv, int32_t bi, const double* v_host, double scalar, const double* r_host,
                           double out_host[2], int max_wgs = 0);
// trmm.hip: out (n x s, C-order, logical rows) = shift[:, None] + L Z for the lower factor of a fully factored single-GPU matrix
// (kc_force = 1, 2, 4 or 8, from the test hook only: the chunk size, instead of the one the size and the CU count choose)
int factor_matmul(lpgp_ctx* ctx, lpgp_mat* mat, const double* Z_host, int64_t s, const double* shift_host, double* out_host, int kc_force = 0);

// assemble.hip ----------------------------------------------------------------------------
// Every assembly kernel writes element (row_off + i, col_off + j) of the GLOBAL padded matrix to where `lay` keeps
// it on this rank -- or not at all if another rank owns it (single GPU: the identity layout).
int launch_assemble(lpgp_ctx* ctx, hipStream_t stream, const DevDesc& host_desc, const double* x0,
                    int64_t n0, int64_t n0_pad, const double* x1, int64_t n1, int64_t n1_pad,
                    double* out, int64_t ld, int64_t row_off, int64_t col_off, int lower_only,
                    const Layout2D& lay = Layout2D());
// several blocks with ONE descriptor (a block row of a conditioning, the rows of a cross-covariance) in one launch
struct AsmJob {
  const double* x0; int64_t n0, n0_pad;
  const double* x1; int64_t n1, n1_pad;
  int64_t row_off, col_off;
  int lower_only;
};
// one block  sum_p diag(w0[a_p]) (kd_p)(X0, X1) diag(w1[b_p])  of a variable-coefficient operator pair; waits for the stream
int assemble_weighted(lpgp_ctx* ctx, hipStream_t stream, const lpgp_wpair* pairs, int npairs, const double* w0_host, int A0,
                      const double* w1_host, int A1, const lpgp_pts* X0, const lpgp_pts* X1, bool sym, double* out, int64_t ld,
                      int64_t row_off, int64_t col_off, const Layout2D& lay);
int assemble_mixed(lpgp_ctx* ctx, hipStream_t stream, const DevDesc& host_desc, const lpgp_pts* X0, const lpgp_mix* M0, const lpgp_pts* X1,
                   const lpgp_mix* M1, bool sym, double* out, int64_t ld, int64_t row_off, int64_t col_off, const Layout2D& lay);
bool assemble_same_fast(const DevDesc& p, const DevDesc& q);
int launch_assemble_batch(lpgp_ctx* ctx, hipStream_t stream, const DevDesc& host_desc, const AsmJob* jobs, int njobs, double* out, int64_t ld,
                          const Layout2D& lay);
int launch_assemble_kron(lpgp_ctx* ctx, hipStream_t stream, const lpgp_kdesc* kd, int ngroups,
                         const double* const* F0, const int64_t* n0d, const double* const* F1, const int64_t* n1d,
                         double* work, size_t work_doubles, double* out, int64_t ld, int64_t row_off,
                         int64_t col_off, int lower_only, const Layout2D& lay);
size_t kron_work_doubles(int D, const int64_t* n0d, const int64_t* n1d);
constexpr int MV_RHS = 4;         // right-hand sides per pass of the matrix-free product (== MV_R in assemble.hip)
bool kron_fits(const lpgp_kdesc* kd, int ngroups);
// v: [r][v_stride] (0: n1_pad), out: [r][out_stride] (0: n0_pad); accumulate: out += instead of =
int launch_matvec(lpgp_ctx* ctx, hipStream_t stream, const DevDesc& host_desc, const double* x0, int64_t n0,
                  int64_t n0_pad, const double* x1, int64_t n1, int64_t n1_pad, const double* v, int nr,
                  double* part, int splits, double* out, int64_t v_stride = 0, int64_t out_stride = 0, int accumulate = 0);
int launch_add_diag(hipStream_t stream, double* a, int64_t ld, int64_t off, int64_t n, const double* v, double scalar,
                    const Layout2D& lay = Layout2D());
int launch_add_dense(hipStream_t stream, double* a, int64_t ld, int64_t off, int64_t n, const double* b,
                     const Layout2D& lay = Layout2D());

}  // namespace lpgp
