// map_post_internal.h -- what map_post.hip (dazim_map_posterior, one dense block per period), model_post.hip
// (dazim_model_posterior, one dense block for the whole 3-D model) and tradeoff.hip (dazim_model_tradeoff and dazim_map_tradeoff,
// those blocks at every point of a sweep over the regularisation weights) share: the sizes of the dense kernels, their two tile
// forms, the fixed-order sum of a workgroup, the two Gram accumulators (mp_accum_rows over a period's row list, mo_accum_row over a
// column of the transpose), and the host driver of the dense part (map_post_dense.hip), which every entry calls -- so a block of
// the maps and the block of the model go through the same kernels in the same order, bit for bit.  The two posterior entries share
// what follows an entry of Rm in their row passes too (MpOut, MpRowSum, mp_fill_nan, the trace kernel) and their host side's
// argument checks and output buffers (dz_post_check_args, MpOutBufs).
#pragma once
#include <cmath>
#include <vector>

#include "sparse_internal.h"

constexpr int MP_NB = 32;   // panel width of the factorisation and of the inverse (stat map_post.nb)
constexpr int MP_TS = 64;   // the tile kernels' output tile, MP_TS x MP_TS per workgroup of MP_TB threads
constexpr int MP_TB = 256;
constexpr int MP_LD = MP_TS + 1;

typedef double mp_v4 __attribute__((ext_vector_type(4)));

// the two tile forms of acc (+/-)= sum_k As[k][i] Bs[k][j] over a k-major pair of LDS slabs of MP_NB rows.
// plain: thread (ty, tx) holds rows ty + 16u, columns tx + 16v.  mfma: wavefront w holds rows 16w .. 16w+15 as four 16 x 16 blocks,
// lane l of block cb element reg at row (l >> 4) + 4 reg, column 16 cb + (l & 15); the A operand is negated for a subtraction.
struct MpPlain {
  double acc[4][4];
  int ty, tx;
  __device__ __forceinline__ MpPlain(int t) : ty(t >> 4), tx(t & 15) {}
  __device__ __forceinline__ int row(int u, int) const { return ty + 16 * u; }
  __device__ __forceinline__ int colof(int, int v) const { return tx + 16 * v; }
  template <bool SUB>
  __device__ __forceinline__ void slab(const double (*As)[MP_LD], const double (*Bs)[MP_LD], int nk) {
    for (int k = 0; k < nk; k++) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; u++) a[u] = As[k][ty + 16 * u];
#pragma unroll
      for (int v = 0; v < 4; v++) b[v] = Bs[k][tx + 16 * v];
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
          if (SUB) acc[u][v] -= a[u] * b[v];
          else acc[u][v] += a[u] * b[v];
        }
    }
  }
};
struct MpMfma {
  double acc[4][4];   // [reg][cb]
  int w, l;
  __device__ __forceinline__ MpMfma(int t) : w(t >> 6), l(t & 63) {}
  __device__ __forceinline__ int row(int u, int) const { return 16 * w + (l >> 4) + 4 * u; }
  __device__ __forceinline__ int colof(int, int v) const { return 16 * v + (l & 15); }
  template <bool SUB>
  __device__ __forceinline__ void slab(const double (*As)[MP_LD], const double (*Bs)[MP_LD], int) {   // (rows nk .. MP_NB-1 hold 0)
    mp_v4 d[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
      for (int r = 0; r < 4; r++) d[cb][r] = acc[r][cb];
#pragma unroll
    for (int k0 = 0; k0 < MP_NB; k0 += 4) {
      const double a0 = As[k0 + (l >> 4)][16 * w + (l & 15)], a = SUB ? -a0 : a0;
#pragma unroll
      for (int cb = 0; cb < 4; cb++) d[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[k0 + (l >> 4)][16 * cb + (l & 15)], d[cb], 0, 0, 0);
    }
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r][cb] = d[cb][r];
  }
};

// the sums of a workgroup's MP_TB threads in a fixed order: butterfly inside a wavefront, the wavefronts' values in ascending order
__device__ __forceinline__ double mp_block_sum(double v, double *red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < MP_TB / 64; i++) s += red[i];
  return s;
}

// ---- the row pass of dazim_map_posterior (k_mp_rows) and dazim_model_posterior (k_mo_rows) ------------------------------------------
// The two kernels obtain an entry Rm_ac by different routes (LDS scatter in the maps, transpose gather in the model); the rest is here.
struct MpOut {   // per-unknown outputs (width_h is the maps' width; width_z, leak and rows may be null) and the selected rows of Rm
  float *std_post, *std_noise, *rdiag, *rsum, *width_h, *width_z, *leak, *rows;
};

// One thread's part of what is summed along row a of Rm.  DEPTH: the vertical width too (the model); without it the struct has no
// sixth sum, so the maps' pass keeps five block sums.
template <bool DEPTH>
struct MpRowSum {
  double rs = 0.0, nv = 0.0, own = 0.0, oth = 0.0, numh = 0.0, numz = 0.0;
  // r = Rm_ac, cac = C_ac; same_block: c lies in a's block, dh2 and dz2 its squared horizontal and vertical distance from a
  __device__ __forceinline__ void add(double r, double cac, bool same_block, double dh2, double dz2) {
    rs += r;
    nv += r * cac;
    double o = own, x = oth;   // (locals: a store to own or oth by a selected address would put the struct into scratch)
    if (same_block) {
      o += r * r;
      numh += r * r * dh2;
      if (DEPTH) numz += r * r * dz2;
    } else {
      x += r * r;
    }
    own = o;
    oth = x;
  }
  __device__ __forceinline__ void reduce(double *red) {
    rs = mp_block_sum(rs, red);
    nv = mp_block_sum(nv, red);
    own = mp_block_sum(own, red);
    oth = mp_block_sum(oth, red);
    numh = mp_block_sum(numh, red);
    if (DEPTH) numz = mp_block_sum(numz, red);
  }
  // one thread, after reduce: the outputs of unknown a at o; caa = C_aa, rdiag = Rm_aa
  __device__ __forceinline__ void write(MpOut out, size_t o, double caa, double rdiag, double *rd64, int a) const {
    out.std_post[o] = (float)sqrt(caa);
    out.std_noise[o] = (float)sqrt(fmax(nv, 0.0));
    out.rdiag[o] = (float)rdiag;
    out.rsum[o] = (float)rs;
    if (out.width_h) out.width_h[o] = own > 0.0 ? (float)sqrt(numh / own) : 0.0f;
    if (DEPTH && out.width_z) out.width_z[o] = own > 0.0 ? (float)sqrt(numz / own) : 0.0f;
    if (out.leak) out.leak[o] = own + oth > 0.0 ? (float)(oth / (own + oth)) : 0.0f;
    rd64[a] = rdiag;
  }
};

// unknown a (outputs at o) of a block that could not be factored: NaN in every output, rd64 and a's rows s0 + s of out.rows, n long
__device__ __forceinline__ void mp_fill_nan(MpOut out, size_t o, double *rd64, int a, int t, int nsel, const int *sel, size_t s0, int n) {
  const float v = nanf("");
  if (t == 0) {
    out.std_post[o] = out.std_noise[o] = out.rdiag[o] = out.rsum[o] = v;
    if (out.width_h) out.width_h[o] = v;
    if (out.width_z) out.width_z[o] = v;
    if (out.leak) out.leak[o] = v;
    rd64[a] = (double)v;
  }
  if (out.rows)
    for (int s = 0; s < nsel; s++)
      if (sel[s] == a)
        for (int c = t; c < n; c += MP_TB) out.rows[(s0 + s) * n + c] = v;
}

// local index blk * ncell + cell of column c = blk * kn + p * ncell + cell of the maps' layout (kn = kmax ncell)
__device__ __forceinline__ int mp_local(int c, int kn, int ncell) { return (c / kn) * ncell + c % ncell; }

// One wavefront (lane t) finds, among the rows list[0 .. nrow) of period p, those that hold the local unknown a, in the order of the
// list, and calls f(b, e, v, r) on every lane for each: row r has the entries b .. e and the value v at a's column.  A row of the
// matrix holds column a at most once.  Of 64 rows at a time only those whose range of cells holds a's cell are read (a map row has
// about 130 of 2 704 cells, close together).
template <class F>
__device__ __forceinline__ void mp_rows_with(int a, int t, int ncell, int kn, int p, int nrow, const int *list, const int *span,
                                             const int64_t *rowptr, const int *col, const float *val, F f) {
  const int cell_a = a % ncell, ga = (a / ncell) * kn + p * ncell + a % ncell;
  for (int i0 = 0; i0 < nrow; i0 += 64) {
    long long mb = 0, me = 0;
    int r = 0;
    bool near = false;
    if (i0 + t < nrow) {
      r = list[i0 + t];
      mb = rowptr[r];
      me = rowptr[r + 1];
      near = span[2 * (size_t)r] <= cell_a && cell_a <= span[2 * (size_t)r + 1];
    }
    for (unsigned long long cand = __ballot(near); cand; cand &= cand - 1ull) {   // ascending rows
      const int k = __ffsll((long long)cand) - 1;
      const long long b = __shfl(mb, k), e = __shfl(me, k);
      float va = 0.0f;
      bool hit = false;
      for (long long q = b + t; q < e; q += 64)
        if (col[q] == ga) {
          va = val[q];
          hit = true;
        }
      const unsigned long long h = __ballot(hit);
      if (!h) continue;
      f(b, e, (double)__shfl(va, __ffsll((long long)h) - 1), __shfl(r, k));
    }
  }
}

// One wavefront (lane t) adds to row a of a period's normal matrix, Aa[c] for c <= a in the local index, the rows list[0 .. nrow) of
// period p in the order of the list: Aa[c] += r_a r_c (SCALED: f * (r_a r_c)).  dazim_map_posterior's Gram pass takes all rows of
// the period; dazim_map_tradeoff the data rows once and the regularisation rows per sweep point -- the same numbers added in the
// same order.
template <bool SCALED>
__device__ __forceinline__ void mp_accum_rows(int a, int t, int ncell, int kn, int p, int nrow, const int *list, const int *span,
                                              const int64_t *rowptr, const int *col, const float *val, double f, double *Aa) {
  mp_rows_with(a, t, ncell, kn, p, nrow, list, span, rowptr, col, val, [=](long long b, long long e, double v, int) {
    for (long long q = b + t; q < e; q += 64) {
      const int lc = mp_local(col[q], kn, ncell);
      if (lc <= a) {
        if (SCALED) Aa[lc] += f * (v * (double)val[q]);
        else Aa[lc] += v * (double)val[q];
      }
    }
    __syncthreads();   // (the next row may hold the same columns in other lanes)
  });
}

constexpr int MO_UN = 4;    // row entries per lane in flight in mo_accum_row

// One wavefront (lane t) adds to row a of a normal matrix, Aa[c] for c <= a, the entries [p0, p1) of column a in the transpose, rows
// ascending: Aa[c] += v_a r_c (SCALED: f * (v_a r_c)) for the entries of row r with c <= a.  The columns of a row are distinct, so
// MO_UN x 64 of its entries are in flight at a time; the barrier between two rows orders the read-modify-writes of an element that two
// rows share (it may sit in different lanes).  dazim_model_posterior's Gram pass takes the whole column; dazim_model_tradeoff the data
// rows once and the regularisation rows per sweep point -- the same numbers added in the same order.
template <bool SCALED>
__device__ __forceinline__ void mo_accum_row(int a, int t, int n, int64_t p0, int64_t p1, const int *row, const float *tval,
                                             const int64_t *rowptr, const int *col, const float *val, double f, double *Aa) {
  for (int64_t p = p0; p < p1; p++) {
    const int r = row[p];
    const double v = (double)tval[p];
    const int64_t b = rowptr[r], e = rowptr[r + 1];
    for (int64_t q0 = b; q0 < e; q0 += 64 * MO_UN) {
      if (col[q0] > a) break;                       // (ascending: nothing at or behind q0 is <= a)
      int cc[MO_UN];
      double pr[MO_UN], old[MO_UN];
#pragma unroll
      for (int u = 0; u < MO_UN; u++) {
        const int64_t q = q0 + u * 64 + t;
        cc[u] = q < e ? col[q] : n;
        if (cc[u] > a) cc[u] = -1;
        pr[u] = cc[u] >= 0 ? v * (double)val[q] : 0.0;
        if (SCALED) pr[u] = f * pr[u];
      }
#pragma unroll
      for (int u = 0; u < MO_UN; u++) old[u] = cc[u] >= 0 ? Aa[cc[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < MO_UN; u++)
        if (cc[u] >= 0) Aa[cc[u]] = old[u] + pr[u];
    }
    __syncthreads();
  }
}

// The argument checks the two posterior entries share, in their order, under the entry's name: n_is words the product A->n has
// to equal (n_ok: it does), `coupled` the mode without which there is no leak, `also` a refusal only one entry knows (NULL: none).
static inline int dz_post_check_args(dazim_ctx *ctx, const char *entry, const dazim_csr *A, int64_t m_data, bool n_ok, const char *n_is, int64_t n_want,
                                     bool is_coupled, const char *coupled, const float *leak_u, const char *also, float damp, int nsel,
                                     const int *sel_u, const float *rows_u) {
  if (m_data < 0 || m_data > A->m) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: m_data %lld outside 0..%lld", entry, (long long)m_data, (long long)A->m);
  if (!n_ok) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: n %lld is not %s = %lld", entry, (long long)A->n, n_is, (long long)n_want);
  if (!is_coupled && leak_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: leak without %s", entry, coupled);
  if (also) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: %s", entry, also);
  if (!(damp >= 0.0f) || !std::isfinite(damp)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: damp negative or not finite", entry);
  if (nsel < 0 || (nsel > 0 && !sel_u)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: nsel without sel", entry);
  if (rows_u && nsel < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: rows without sel", entry);
  return 0;
}

// The outputs of a posterior entry, each where the user keeps it (host or device): `no` values per unknown, nrows * no_row of the
// selected rows, ntrace of the trace; an output the user did not ask for has no buffer.
struct MpOutBufs {
  DzBuf<float> sp, sn, rd, rs, wh, wz, lk, rw, tr;
  int init(dazim_ctx *ctx, float *std_post_u, float *std_noise_u, float *rdiag_u, float *rsum_u, float *width_h_u, float *width_z_u, float *leak_u,
           float *rows_u, float *trace_u, size_t no, size_t nrows, size_t ntrace) {
    int rc;
    if ((rc = sp.init(ctx, std_post_u, no, false, true)) || (rc = sn.init(ctx, std_noise_u, no, false, true)) ||
        (rc = rd.init(ctx, rdiag_u, no, false, true)) || (rc = rs.init(ctx, rsum_u, no, false, true)) ||
        (rc = wh.init(ctx, width_h_u, width_h_u ? no : 0, false, true)) || (rc = wz.init(ctx, width_z_u, width_z_u ? no : 0, false, true)) ||
        (rc = lk.init(ctx, leak_u, leak_u ? no : 0, false, true)) || (rc = rw.init(ctx, rows_u, rows_u ? nrows : 0, false, true)) ||
        (rc = tr.init(ctx, trace_u, trace_u ? ntrace : 0, false, true)))
      return rc;
    return 0;
  }
  MpOut dev() const { return {sp.dev, sn.dev, rd.dev, rs.dev, wh.dev, wz.dev, lk.dev, rw.dev}; }
  int finish() {
    for (DzBuf<float> *b : {&sp, &sn, &rd, &rs, &wh, &wz, &lk, &rw, &tr})
      if (int rc = b->finish()) return rc;
    return 0;
  }
};

#pragma GCC visibility push(hidden)
// map_post.hip: trace[b * stride + off] = sum of rd64[b * ncell .. (b+1) * ncell) for b < nb, one workgroup each, enqueued on the
// context's stream without a check of its own.  The maps call it per period p with (kmax, p), the model once with (1, 0).
void dz_mp_trace(dazim_ctx *ctx, int nb, int ncell, int stride, int off, const double *rd64, float *trace);
// dz_mp_dense's two halves: the factorisation alone (seconds ADDED to sec[0]), and inverse and C (sec[1], sec[2]).  dz_mp_dense is
// the first followed by the second: the same launches in the same order.
int dz_mp_factor(dazim_ctx *ctx, int ng, double *Ad, int *flag, bool mfma, const char *lap, double *sec);
int dz_mp_inverse_c(dazim_ctx *ctx, int ng, double *Ad, double *Cd, bool mfma, const char *lap, double *sec);
// model_post.hip: *bad (device) |= 1 when a row's columns do not ascend strictly inside 0..n-1; regstart[c] = the first entry of column c
// in the transpose that belongs to a row >= m_data.  Both enqueue on the context's stream.
int dz_mo_check_rows(dazim_ctx *ctx, const dazim_csr *A, int n, int *bad);
int dz_mo_regstart(dazim_ctx *ctx, const dazim_csr *A, int n, int64_t m_data, int64_t *regstart);
// The dense part on one block of ng unknowns, enqueued on the context's stream: Ad [ng][ng] holds the lower triangle of the normal
// matrix and ends as M = R^-1 (lower triangle), Cd [ng][max(ng, MP_NB)] is scratch for the inverse and ends as C = M^T M, both
// triangles; *flag (device) is set to 1 at a pivot that is not finite and > 0.  mfma: the tile form of the trailing update and of C.
// The seconds of factor, inverse and C are ADDED to sec[0..2]; they are measured with the context's events under the stat `lap`.
int dz_mp_dense(dazim_ctx *ctx, int ng, double *Ad, double *Cd, int *flag, bool mfma, const char *lap, double *sec);
// map_post.hip, the rows of every period of the maps' layout (kn = kmax ncell), on the context's stream: per [m] the period of a row
// (-1: no entries), span [2m] the range of cells it touches, list [m] the rows period by period, ascending; cnt [2 kmax + 1] (device)
// and hcnt (host, after a synchronisation) the rows and the data rows of period p at 2p, 2p + 1, and at 2 kmax the bits 1 (a row in two
// periods) and 2 (columns that do not ascend strictly).  With a bit set the list is not written.
int dz_mp_period_rows(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, int kmax, int kn, int ncell, int *per, int *span, int *cnt, int *list,
                      std::vector<int> &hcnt);
// k_mp_gram on the rows list[0 .. nrow) of period p: the lower triangle of sum_r r^T r + d2 I into Ad [ng][ng], zeros above it
int dz_mp_gram(dazim_ctx *ctx, int ng, int ncell, int kn, int p, int nrow, const int *list, const int *span, const dazim_csr *A, double d2, double *Ad);
#pragma GCC visibility pop
