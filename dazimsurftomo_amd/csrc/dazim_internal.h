// dazim_internal.h -- shared plumbing of libdazim_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dazim.h"

struct dazim_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string err;
  std::map<std::string, double> ksec;  // last measured kernel seconds by name
  int num_cu = 256;
  std::map<std::string, int> opts;     // dazim_set_option
  // reusable device scratch, grown on demand (never shrunk) so that repeated calls do not hipMalloc
  std::map<std::string, std::pair<void *, size_t>> scratch;
  // pinned host buffers by name (dz_pinned): where the step's small device-to-host reads land -- a copy into pageable memory is
  // staged by a blit KERNEL, which waits for a free wavefront slot behind persistent workgroups (the dispersion copies held the
  // chip for 20 ms while a 4-byte read waited, profiles/r5); into pinned memory it is a DMA transfer
  std::map<std::string, std::pair<void *, size_t>> pinned;
  bool fmm_busy = false;   // an eikonal call is using its scratch blocks (dz_trim_caches must not free them)
  // RCCL communicator of a row-sharded solve (dazim_comm_init); nullptr = single GPU, RCCL never touched
  // staging blocks for host-pointer arguments (DzBuf): released blocks are kept and handed out again, because a
  // hipMalloc + hipFree pair per staged array costs milliseconds in a program that calls the library once per outer iteration
  struct StageBlock { void *p; size_t bytes; bool busy; };
  std::vector<StageBlock> stage;
  // matrix arrays (CSR values / columns / row pointers of G, hundreds of MB to GB each): a program builds and frees one G per
  // outer iteration, and a hipMalloc + hipFree pair of that size costs about a millisecond each -- freed arrays are kept
  // (a few, best fit) and handed out again
  std::vector<StageBlock> big;
  // auxiliary stream (option disp.async): the perturbed copies of the dispersion kernel run there while the main stream goes on
  // with the column's own curves, the gridder and the eikonal fields; whoever consumes the depth kernels joins first (dz_join_aux)
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_a0 = nullptr, ev_a1 = nullptr;
  bool aux_pending = false, aux_timed = false;
  // device ranges the auxiliary stream's pending work reads or writes (the model and the three kernel tables): a host copy that
  // touches none of them does not have to wait for it (dazim_memcpy_h2d / _d2h)
  struct AuxRange { const char *p; size_t bytes; };
  std::vector<AuxRange> aux_ranges;
  // what the join of the auxiliary stream still has to do on the MAIN stream (dazim_dispersion_kernels_sharded: the all-gather
  // of the ranks' blocks of the depth-kernel tables); run once by dz_join_aux / dazim_sync, dropped by dazim_destroy
  int (*aux_epilogue)(dazim_ctx *) = nullptr;
  struct ShardPending {
    int nx = 0, ny = 0, nz = 0, kmax = 0;
    const double *send = nullptr;                     // this rank's blocks of sen_vs | sen_vp | sen_rho
    double *svs = nullptr, *svp = nullptr, *srho = nullptr;   // the complete tables (device)
  } shard;
  // eikonal fields a dazim_fmm_batch call with ttn == NULL left inside the library for dazim_rays_build_G* with ttn == NULL: the
  // finished node words of every field in the eikonal kernel's own 4 x 4 tiles (scratch "fmm.rec_c" / "fmm.ttn_tiled", which
  // dz_trim_caches leaves alone while `tiled` is set); field f at tiled + (tslot ? tslot[f] : f) * stride
  struct TiledFields {
    const unsigned *tiled = nullptr;
    const int *tslot = nullptr;
    int nfield = 0, nnx = 0, nnz = 0, stride = 0, tsh = 0;
    const int *fdone = nullptr;   // asynchronous eikonal call: per field 0 = still marching, 1 = finished, 2 = band overflow (rerun pending)
    unsigned nwg = 0;                    // workgroups of that launch
    volatile unsigned *hprog = nullptr;  // host-mapped: tasks handed out so far per XCD range of the asynchronous launch, of total_tasks:
    unsigned total_tasks = 0;            // the ray call launches its count pass when the queue is nearly empty (not before: see rays.hip)
  } fields;
  // Option fmm.async (with ttn == NULL, device-resident arguments and a time-sliced batch): dazim_fmm_batch returns when its launch
  // is enqueued, and the dazim_rays_build_G* call that follows runs its count pass on a third stream as non-blocking passes over
  // the quads of rays whose fields' completion flags are set -- its workgroups are dispatched as the eikonal launch's persistent
  // workgroups leave: the ray kernel fills the TAIL of the eikonal launch (profiles/r6_tail_fill.md).  fmm_finish = what the
  // eikonal call still owes (FmmBatch::finish of fmm.hip; the closure holds the batch); run by the ray call, by dazim_sync / dazim_free / a copy / the next
  // eikonal or dispersion call, whichever comes first (dz_fmm_finish).
  std::function<int()> fmm_finish;
  unsigned *hprog = nullptr;           // pinned, device-visible: 8 progress words of an asynchronous eikonal launch (dz_async_init)
  hipStream_t stream3 = nullptr;
  hipEvent_t ev_f0 = nullptr, ev_f1 = nullptr, ev_pre = nullptr, ev_r0 = nullptr, ev_r1 = nullptr;
  void *comm = nullptr;
  void (*comm_release)(dazim_ctx *) = nullptr;   // set by dazim_comm_init: dazim_destroy must not leak the communicator
  int nranks = 1, rank = 0;
};

int dz_fail(dazim_ctx *c, int code, const char *fmt, ...);
// value of an option, `def` where it was never set (the look-up does not insert it)
static inline int dz_opt(const dazim_ctx *ctx, const char *name, int def) {
  const auto it = ctx->opts.find(name);
  return it == ctx->opts.end() ? def : it->second;
}

// ---- the communicator of a multi-rank run (comm.hip) ---------------------------------------------------------------------------
struct DzComm {
  ncclComm_t nccl = nullptr;
  std::string dir;        // non-empty: the file transport (tests: several ranks on ONE GPU)
  std::string tag;        // ... the nonce every file of this communicator carries in its name
  unsigned seq = 0;
  int nranks = 1, rank = 0;
};
enum { DZ_F32 = 0, DZ_F64 = 1, DZ_I64 = 2, DZ_SUM = 0, DZ_MAX = 1 };
// recv[r*bytes .. (r+1)*bytes) = rank r's `bytes` bytes at send, every rank the same; DEVICE buffers, on the context's stream
int dz_allgather(dazim_ctx *ctx, DzComm *c, const void *send_dev, void *recv_dev, size_t bytes);
// in-place sum / max over the ranks of a DEVICE buffer on the context's stream: all-gather + one kernel that combines the ranks'
// values in RANK ORDER (the same bits on every rank, with every transport and every rank count's grouping)
int dz_allreduce(dazim_ctx *ctx, DzComm *c, void *dbuf, size_t count, int dtype, int op);
// a rank that fails on its own after the others may already wait in a collective: abort the communicator, detach it
void dz_comm_abort(dazim_ctx *ctx);
// even contiguous split of n items over the ranks (dazim_shard_rows of host/dazim_mod.f90, shard_rows of distributed.py)
static inline void dz_shard_even(int64_t n, int world, int rank, int64_t *lo, int64_t *hi) {
  const int64_t base = n / world, rem = n % world;
  *lo = rank * base + (rank < rem ? rank : rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
}

#define DZ_NCCL(call)                                                                                        \
  do {                                                                                                        \
    ncclResult_t r_ = (call);                                                                                 \
    if (r_ != ncclSuccess) return dz_fail(ctx, -2000 - (int)r_, "%s:%d %s -> %s", __FILE__, __LINE__, #call, ncclGetErrorString(r_)); \
  } while (0)
int dz_aux_init(dazim_ctx *ctx);                  // creates the auxiliary stream and its events on first use
int dz_async_init(dazim_ctx *ctx);                // ... the third stream and the events of an asynchronous eikonal call
int dz_fmm_finish(dazim_ctx *ctx);                // completes a pending asynchronous eikonal call (no-op without one)
int dz_join_aux(dazim_ctx *ctx);                  // main stream waits for what the auxiliary stream was given (no host wait)
int dz_join_aux_if_touched(dazim_ctx *ctx, const void *dev, size_t bytes);   // ... only if [dev, dev + bytes) overlaps what it works on

#define DZ_HIP(call)                                                                           \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return dz_fail(ctx, -(int)e_ - 1000, "%s:%d %s -> %s", __FILE__, __LINE__, #call,       \
                     hipGetErrorString(e_));                                                   \
  } while (0)

// The eikonal kernel's 4 x 4-tile layout of a grid (described in fmm.hip; the ray kernel reads the finished fields through it):
// node (x0, z0), 0-based, is word dz_tile_x(x0, tsh) + dz_tile_z(z0), tsh = dz_tile_shift(nnz); a field takes dz_tile_records words
__host__ __device__ constexpr int dz_tile_shift(int nz) { int l = 0; while ((1 << l) < ((nz + 3) >> 2)) l++; return l + 4; }
__host__ __device__ constexpr int dz_tile_records(int nx, int nz) { return ((nx + 3) >> 2) << dz_tile_shift(nz); }
__host__ __device__ __forceinline__ constexpr int dz_tile_x(int x0, int tsh) { return ((x0 >> 2) << tsh) + ((x0 & 3) << 2); }
__host__ __device__ __forceinline__ constexpr int dz_tile_z(int z0) { return ((z0 & ~3) << 2) | (z0 & 3); }

// The factor of a dVs row entry that does not depend on the ray (inv/CalSurfG.f90:1339-1364): dc/dVs of a model cell for one period,
// the Brocher derivatives coe_a, coe_rho of the cell's velocity v and its three depth kernels, (svp*coe_a + srho*coe_rho + svs) in
// the reference's order and precision.  k_row_kernels (rays.hip, the table the 3-D rows multiply) and dazim_vs_kernels (column.hip)
// both call it, so the two tables are the same bits.
__device__ __forceinline__ double dz_row_kernel(float v, double svs, double svp, double srho) {
  const float coe_a = (2.0947f - 0.8206f * 2 * v + 0.2683f * 3 * (v * v) - 0.0251f * 4 * (v * v * v));
  const float vpft = 0.9409f + 2.0947f * v - 0.8206f * (v * v) + 0.2683f * (v * v * v) - 0.0251f * (v * v * v * v);
  const float coe_rho = coe_a * (1.6612f - 0.4721f * 2 * vpft + 0.0671f * 3 * (vpft * vpft) -
                                 0.0043f * 4 * (vpft * vpft * vpft) + 0.000106f * 5 * (vpft * vpft * vpft * vpft));
  return svp * (double)coe_a + srho * (double)coe_rho + svs;
}

// entry (a, b) of L^T L for L the depth rule of TikhRegul (inv/TikhRegul.f90:2) restricted to one column of n knots: the first
// and the last row hold the single entry 2, an inner row i holds 2 at i and -1 at i - 1 and i + 1
__device__ __forceinline__ double dz_ltl(int n, int a, int b) {
  auto L = [n](int i, int c) -> double {
    if (i == 0 || i == n - 1) return c == i ? 2.0 : 0.0;
    return c == i ? 2.0 : ((c == i - 1 || c == i + 1) ? -1.0 : 0.0);
  };
  double s = 0.0;
  const int lo = max(max(a, b) - 1, 0), hi = min(min(a, b) + 1, n - 1);
  for (int i = lo; i <= hi; i++) s += L(i, a) * L(i, b);
  return s;
}

// The regularised column problem of dazim_column_lsq for one wavefront (lane t of 64) on its LDS arrays:
// from K [kmax][n], w^2 [kmax] and w^2 r [nrhs][kmax] the normal matrix A = K^T W^2 K + s2 L^T L + d2 I (lower triangle of
// A [n][n]) and b_r = K^T W^2 r_r, the right-looking Cholesky A = R R^T (R replaces the lower triangle; the strict upper triangle
// of A is never touched) and the two substitutions per right-hand side, which leave the solutions in b [nrhs][n].  fp64, every
// sum in a fixed order.  The caller has filled K, w2 and wr and passed a barrier.  Returns whether every pivot was finite and
// > 0 (the same on every lane); the arithmetic does not depend on it.  k_column_lsq (column.hip) and k_mc_aniso (column_mc.hip)
// both call it, so a cell's Gc/Gs from the depth program and the conditional mean of the Monte-Carlo program are the same bits.
__device__ __forceinline__ bool dz_column_solve(int t, int n, int kmax, int nrhs, double *A, const double *K, const double *w2,
                                                const double *wr, double *b, double s2, double d2) {
  constexpr int W = 64;
  for (int q = t; q < n * n; q += W) {            // lower triangle of the normal matrix
    const int a = q / n, c = q - a * n;
    if (c > a) continue;
    double s = 0.0;
    for (int p = 0; p < kmax; p++)
      if (w2[p] != 0.0) s += w2[p] * K[p * n + a] * K[p * n + c];
    s += s2 * dz_ltl(n, a, c);
    if (a == c) s += d2;
    A[q] = s;
  }
  for (int q = t; q < nrhs * n; q += W) {
    const int r = q / n, a = q - r * n;
    double s = 0.0;
    for (int p = 0; p < kmax; p++)
      if (w2[p] != 0.0) s += wr[r * kmax + p] * K[p * n + a];
    b[q] = s;
  }
  __syncthreads();
  bool ok = true;
  for (int c = 0; c < n; c++) {                   // right-looking Cholesky, column c
    const double p = A[c * n + c];
    ok = ok && isfinite(p) && p > 0.0;
    const double d = sqrt(p);
    if (t > c && t < n) A[t * n + c] /= d;
    __syncthreads();
    if (t == c) A[c * n + c] = d;
    const int m = n - c - 1;
    for (int q = t; q < m * m; q += W) {
      const int a = c + 1 + q / m, e = c + 1 + q % m;
      if (e <= a) A[a * n + e] -= A[a * n + c] * A[e * n + c];
    }
    __syncthreads();
  }
  for (int r = 0; r < nrhs; r++) {
    double *br = b + r * n;
    for (int c = 0; c < n; c++) {                 // L y = b
      const double y = br[c] / A[c * n + c];
      __syncthreads();
      if (t > c && t < n) br[t] -= A[t * n + c] * y;
      if (t == c) br[c] = y;
      __syncthreads();
    }
    for (int c = n - 1; c >= 0; c--) {            // L^T x = y
      const double y = br[c] / A[c * n + c];
      __syncthreads();
      if (t < c) br[t] -= A[c * n + t] * y;
      if (t == c) br[c] = y;
      __syncthreads();
    }
  }
  return ok;
}

// Column k of the inverse factor M = R^-1 of dz_column_solve's A = R R^T, formed by lane k alone by forward substitution on e_k:
// y_k = 1 / R_kk, y_i = -(sum_{j=k..i-1} R_ij y_j) / R_ii.  y_i for i > k goes to A[k*n + i], the strict upper triangle of A that the
// factorisation never touches (row k belongs to lane k, so the lanes need no barrier among themselves); the diagonal keeps R_kk.
// Returns (A^-1)_kk = sum_{i=k..n-1} y_i^2 in ascending i.  k_mc_aniso (column_mc.hip) and k_column_res (column.hip) both call it,
// so the Monte-Carlo pass's conditional variance and the depth program's posterior variance are the same bits.
__device__ __forceinline__ double dz_column_inverse_factor(int k, int n, double *A) {
  const double yk = 1.0 / A[k * n + k];
  double dg = yk * yk;
  for (int i = k + 1; i < n; i++) {
    double s = A[i * n + k] * yk;
    for (int j = k + 1; j < i; j++) s += A[i * n + j] * A[k * n + j];
    const double yi = -s / A[i * n + i];
    A[k * n + i] = yi;
    dg += yi * yi;
  }
  return dg;
}

// The RMS statistics of a column solve (column.hip), enqueued on the context's stream: out [nrp][2] = per (right-hand side, period)
// rp the RMS over the cells with wdat [kmax][ncell] != 0 (NULL: all) of r and of r - K x, from the solve kernel's partial sums
// part [nrp][ncell][2], period rp % kmax, in a fixed order.  dazim_column_lsq and dazim_column_lsq_radial (once per wave type) call it.
int dz_column_stats(dazim_ctx *ctx, int ncell, int nrp, int kmax, const float *wdat, const double *part, float *out);

// The refined layer table of a column model, refineGrid2LayerMdl (inv/CalSurfG.f90:2339-2365) in its fp32 expressions: the interval
// between knots i and i + 1 (iv = i, 1-based) becomes nsub sublayers, sublayer j with the weights fm / den = (2j - 1) / (2 nsub) and the
// thickness thk; the last row is the half-space (iv = 0).  dazim_dispersion_kernels and dazim_ti_kernels build their tables on it.
struct DzRefinedLayer { int iv; float fm, den, thk; };
static inline std::vector<DzRefinedLayer> dz_refine_layers(const float *depz, int nz, float minthk0) {
  std::vector<DzRefinedLayer> lay;
  for (int i = 1; i <= nz - 1; i++) {
    const float thk = depz[i] - depz[i - 1], minthk = thk / minthk0;
    const int nsub = (int)((thk + 1.0e-4f) / minthk) + 1;
    for (int j = 1; j <= nsub; j++) lay.push_back({i, (float)(2 * j - 1), (float)(2 * nsub), thk / (float)nsub});
  }
  lay.push_back({0, 0.0f, 1.0f, 0.0f});
  return lay;
}

// named scratch buffer of at least `bytes` bytes
int dz_scratch(dazim_ctx *ctx, const char *name, size_t bytes, void **out);
// named PINNED host buffer of at least `bytes` bytes (measured neutral against pageable memory, profiles/r6_pinned_ab.md)
int dz_pinned(dazim_ctx *ctx, const char *name, size_t bytes, void **out);

size_t dz_trim_caches(dazim_ctx *ctx);                                // free all idle cached blocks; bytes released
hipError_t dz_malloc_retry(dazim_ctx *ctx, void **p, size_t bytes);   // hipMalloc; on out-of-memory trim the caches and retry once
bool dz_is_device_ptr(const void *p);
int dz_stage_get(dazim_ctx *ctx, size_t bytes, void **out);   // a device block of >= bytes from the context's staging cache
void dz_stage_put(dazim_ctx *ctx, void *p);                   // give it back (kept for reuse; freed by dazim_destroy)
int dz_big_get(dazim_ctx *ctx, size_t bytes, void **out);     // a device array for a matrix (see dazim_ctx::big)
void dz_big_put(dazim_ctx *ctx, void *p);                     // return it (any hipMalloc'ed pointer is accepted; ctx may be null)
// dz_scratch / dz_big_get for `count` elements of T
template <class T>
static inline int dz_scratch(dazim_ctx *ctx, const char *name, size_t count, T **out) {
  void *p = nullptr;
  const int rc = dz_scratch(ctx, name, count * sizeof(T), &p);
  *out = (T *)p;
  return rc;
}
template <class T>
static inline int dz_big_get(dazim_ctx *ctx, size_t count, T **out) {
  void *p = nullptr;
  const int rc = dz_big_get(ctx, count * sizeof(T), &p);
  *out = (T *)p;
  return rc;
}

// take ownership of device CSR arrays whose allocations hold cap_m rows / cap_nnz entries (0 = exactly m / nnz); sparse.hip
extern "C" int dz_csr_adopt_cap(dazim_ctx *ctx, int64_t m, int64_t n, int64_t nnz, int64_t *rowptr, int *col, float *val,
                                int64_t cap_m, int64_t cap_nnz, dazim_csr **out);

// attach B as the "dense twin" of A (A owns it until dazim_csr_take_twin hands it out; dazim_csr_free(A) frees an attached twin)
extern "C" int dz_csr_set_twin(dazim_ctx *ctx, dazim_csr *A, dazim_csr *B);

// every a[i] of a DEVICE array inside lo..hi?  Returns 0, or DAZIM_E_BAD_ARG with "<what> outside lo..hi" as the message.
int dz_check_range(dazim_ctx *ctx, const int *a_dev, int64_t n, int lo, int hi, const char *what);

// Staging helper: wraps a user pointer that may live on the host or on the device.
template <class T>
struct DzBuf {
  dazim_ctx *ctx = nullptr;
  T *user = nullptr;
  T *dev = nullptr;
  size_t n = 0;
  bool staged = false, out = false;
  int init(dazim_ctx *c, const T *p, size_t count, bool copy_in, bool copy_out) {
    ctx = c;
    user = const_cast<T *>(p);
    n = count;
    out = copy_out;
    if (!p || count == 0) return 0;
    if (dz_is_device_ptr(p)) {
      dev = user;
      return 0;
    }
    staged = true;
    {
      void *blk = nullptr;
      int rc_ = dz_stage_get(ctx, n * sizeof(T), &blk);
      if (rc_) return rc_;
      dev = (T *)blk;
    }
    if (copy_in) DZ_HIP(hipMemcpyAsync(dev, user, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return 0;
  }
  int finish() {
    if (staged && out && dev)
      DZ_HIP(hipMemcpyAsync(user, dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
  }
  ~DzBuf() {
    if (staged && dev) {
      (void)hipStreamSynchronize(ctx->stream);
      dz_stage_put(ctx, dev);
    }
  }
};

// time a region on the ctx stream with HIP events and record it under `name`
struct DzTimer {
  dazim_ctx *ctx;
  const char *name;
  DzTimer(dazim_ctx *c, const char *n) : ctx(c), name(n) { (void)hipEventRecord(ctx->ev0, ctx->stream); }
  void stop() {
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    (void)hipEventSynchronize(ctx->ev1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->ksec[name] = ms * 1e-3;
  }
  void lap(double &sum) {   // stop, and add the seconds to those of a part of the call
    stop();
    sum += ctx->ksec[name];
  }
};

// the seconds of a call's parts, sec[0 .. count), published under names[] and their sum under `total`; the lap stat they were
// measured under is erased
static inline void dz_publish_laps(dazim_ctx *ctx, const char *lap, const char *const *names, const double *sec, int count, const char *total) {
  ctx->ksec.erase(lap);
  double sum = 0.0;
  for (int i = 0; i < count; i++) {
    ctx->ksec[names[i]] = sec[i];
    sum += sec[i];
  }
  ctx->ksec[total] = sum;
}

// up to three device allocations that belong to one call: released on every way out
struct DzOwned {
  void *p[3] = {nullptr, nullptr, nullptr};
  ~DzOwned() {
    for (void *q : p)
      if (q) (void)hipFree(q);
  }
};

// A call whose workspace of `need` bytes has to fit the card before its first launch: where it does not, the caches are trimmed, and
// where it still does not the call is refused with "<entry>: <count> <what> need x GiB of device memory, y GiB are free".
static inline int dz_need_device_bytes(dazim_ctx *ctx, size_t need, const char *entry, long long count, const char *what) {
  size_t fre = 0, tot = 0;
  DZ_HIP(hipMemGetInfo(&fre, &tot));
  if (need > fre) {
    (void)dz_trim_caches(ctx);
    DZ_HIP(hipMemGetInfo(&fre, &tot));
  }
  if (need > fre)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: %lld %s need %.1f GiB of device memory, %.1f GiB are free", entry, count, what,
                   (double)need / 1073741824.0, (double)fre / 1073741824.0);
  return 0;
}
