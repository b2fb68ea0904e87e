// map_post.hip -- dazim_map_posterior: posterior std and resolution of the per-period maps from the matrix LSMR
// is given, [W G; L], and the damping.  The normal matrix is block diagonal by period; per period (group) of n_g unknowns:
//   gram     A_g = sum_rows r^T r + damp^2 I, one wavefront per row of A_g over the period's sparse rows in ascending order
//   factor, inverse, c   the dense part, dz_mp_dense (map_post_dense.hip), which dazim_model_posterior shares: A_g = R R^T in place,
//            M = R^-1 in place, C = M^T M into the second matrix
//   rows     one workgroup per row of Rm = I - C P with the regularisation rows as they are, and every per-unknown output
// fp64, every sum in a fixed order, no floating-point atomics; the dependencies between the steps are launch order on the context's
// stream.  The dense part has two tile forms: plain VALU arithmetic and v_mfma_f64_16x16x4_f64 (option map_post.mfma).
#include <algorithm>
#include <cmath>

#include "map_post_internal.h"

namespace {

constexpr int MP_EMAX = 8;  // entries of a regularisation row the row pass keeps in LDS (a longer row is read from memory again)

// period of every row (-1: a row without entries) and the range of cells it touches, span[2r] .. span[2r+1]; bad |= 1 for a row whose
// columns lie in two periods, |= 2 for a row whose columns do not ascend strictly
__global__ __launch_bounds__(MP_TB) void k_mp_row_period(int64_t m, const int64_t *rowptr, const int *col, int kn, int ncell, int *per,
                                                         int *span, int *bad) {
  const int64_t r = (int64_t)blockIdx.x * MP_TB + threadIdx.x;
  if (r >= m) return;
  int p = -1, prev = -1, b = 0, lo = ncell, hi = -1;
  for (int64_t q = rowptr[r]; q < rowptr[r + 1]; q++) {
    const int c = col[q], pp = (c % kn) / ncell, cell = c % ncell;
    if (p < 0) p = pp;
    else if (pp != p) b |= 1;
    if (c <= prev) b |= 2;
    prev = c;
    lo = min(lo, cell);
    hi = max(hi, cell);
  }
  per[r] = p;
  span[2 * r] = lo;
  span[2 * r + 1] = hi;
  if (b) atomicOr(bad, b);
}

// block p: the rows of period p in ascending order.  list == NULL: cnt[2p] = their number, cnt[2p+1] = how many are data rows;
// otherwise the rows go to list + sum_{q<p} cnt[2q]
__global__ __launch_bounds__(MP_TB) void k_mp_row_lists(int64_t m, int64_t m_data, const int *per, int *cnt, int *list) {
  __shared__ int ws[MP_TB / 64], wd[MP_TB / 64];
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  int base = 0, based = 0, off = 0;
  if (list)
    for (int q = 0; q < p; q++) off += cnt[2 * q];
  for (int64_t r0 = 0; r0 < m; r0 += MP_TB) {
    const int64_t r = r0 + t;
    const bool f = r < m && per[r] == p;
    const unsigned long long bf = __ballot(f), bd = __ballot(f && r < m_data);
    if (lane == 0) {
      ws[w] = __popcll(bf);
      wd[w] = __popcll(bd);
    }
    __syncthreads();
    int wb = 0, tot = 0, totd = 0;
    for (int i = 0; i < MP_TB / 64; i++) {
      if (i < w) wb += ws[i];
      tot += ws[i];
      totd += wd[i];
    }
    if (f && list) list[off + base + wb + __popcll(bf & ((1ull << lane) - 1ull))] = (int)r;
    base += tot;
    based += totd;
    __syncthreads();
  }
  if (!list && t == 0) {
    cnt[2 * p] = base;
    cnt[2 * p + 1] = based;
  }
}

// row a of A_g (all n_g entries; the lower triangle is what the factorisation reads): sum over the period's rows r, ascending, of
// r_a r_c (mp_accum_rows), then damp^2 on the diagonal.  One wavefront per row a.
__global__ __launch_bounds__(64) void k_mp_gram(int ng, int ncell, int kn, int p, int nrow, const int *list, const int *span,
                                                const int64_t *rowptr, const int *col, const float *val, double d2, double *A) {
  const int a = blockIdx.x, t = threadIdx.x;
  double *Aa = A + (size_t)a * ng;
  for (int c = t; c < ng; c += 64) Aa[c] = 0.0;
  __syncthreads();
  mp_accum_rows<false>(a, t, ncell, kn, p, nrow, list, span, rowptr, col, val, 1.0, Aa);
  if (t == 0) Aa[a] += d2;
}

// ---- row pass ----------------------------------------------------------------------------------------------------------------------
// workgroup a: Rm_a. = e_a - sum_l (C_a. l) l - damp^2 C_a. over the period's regularisation rows l in ascending order, and what is
// summed along that row.  Dynamic LDS: rm [ng] | tb [MP_TB] | eval [MP_TB][MP_EMAX] | ebeg [MP_TB] | ecol [MP_TB][MP_EMAX] | elen [MP_TB]
__global__ __launch_bounds__(MP_TB) void k_mp_rows(int ng, int ncell, int nvx, int kn, int p, int nreg, const int *reglist,
                                                   const int64_t *rowptr, const int *col, const float *val, double d2, const double *Cm,
                                                   const int *flag, MpOut out, int nsel, const int *sel, double *rd64) {
  extern __shared__ double sm[];
  __shared__ double red[MP_TB / 64];
  double *rm = sm, *tb = rm + ng, *eval = tb + MP_TB;
  long long *ebeg = (long long *)(eval + MP_TB * MP_EMAX);
  int *ecol = (int *)(ebeg + MP_TB), *elen = ecol + MP_TB * MP_EMAX;
  const int a = blockIdx.x, t = threadIdx.x;
  const int blk = a / ncell, cell = a % ncell;
  const size_t o = (size_t)blk * kn + (size_t)p * ncell + cell;
  if (*flag) {
    mp_fill_nan(out, o, rd64, a, t, nsel, sel, (size_t)p * nsel, ng);
    return;
  }
  const double *Ca = Cm + (size_t)a * ng;
  for (int c = t; c < ng; c += MP_TB) rm[c] = c == a ? 1.0 : 0.0;
  __syncthreads();
  for (int k0 = 0; k0 < nreg; k0 += MP_TB) {
    if (k0 + t < nreg) {
      const int r = reglist[k0 + t];
      const long long b = rowptr[r], e = rowptr[r + 1];
      double s = 0.0;
      for (long long q = b; q < e; q++) {
        const int lc = mp_local(col[q], kn, ncell);
        const double v = (double)val[q];
        s += Ca[lc] * v;
        if (q - b < MP_EMAX) {
          ecol[t * MP_EMAX + (int)(q - b)] = lc;
          eval[t * MP_EMAX + (int)(q - b)] = v;
        }
      }
      tb[t] = s;
      ebeg[t] = b;
      elen[t] = (int)(e - b);
    }
    __syncthreads();
    if (t < 64) {                                   // one wavefront: its LDS operations take effect in program order
      const int nk = min(MP_TB, nreg - k0);
      for (int k = 0; k < nk; k++) {
        const double tt = tb[k];
        const int len = elen[k];
        if (len <= MP_EMAX) {
          if (t < len) rm[ecol[k * MP_EMAX + t]] -= tt * eval[k * MP_EMAX + t];
        } else {
          const long long b = ebeg[k];
          for (int q = t; q < len; q += 64) rm[mp_local(col[b + q], kn, ncell)] -= tt * (double)val[b + q];
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
  }
  for (int c = t; c < ng; c += MP_TB) rm[c] -= d2 * Ca[c];
  __syncthreads();
  const int ia = cell % nvx, ja = cell / nvx;
  MpRowSum<false> sum;
  for (int c = t; c < ng; c += MP_TB) {
    const int cc = c % ncell;
    const double di = (double)(cc % nvx - ia), dj = (double)(cc / nvx - ja);
    sum.add(rm[c], Ca[c], c / ncell == blk, di * di + dj * dj, 0.0);
  }
  sum.reduce(red);
  if (t == 0) sum.write(out, o, Ca[a], rm[a], rd64, a);
  if (out.rows)
    for (int s = 0; s < nsel; s++)
      if (sel[s] == a)
        for (int c = t; c < ng; c += MP_TB) out.rows[((size_t)p * nsel + s) * ng + c] = (float)rm[c];
}

// trace[b * stride + off] = sum of Rm_aa over the ncell unknowns b * ncell .. of workgroup b: the maps' [blk][p], the model's [blk][k]
__global__ __launch_bounds__(MP_TB) void k_mp_trace(int ncell, int stride, int off, const double *rd64, float *trace) {
  __shared__ double red[MP_TB / 64];
  double s = 0.0;
  for (int c = threadIdx.x; c < ncell; c += MP_TB) s += rd64[(size_t)blockIdx.x * ncell + c];
  s = mp_block_sum(s, red);
  if (threadIdx.x == 0) trace[blockIdx.x * stride + off] = (float)s;
}

}  // namespace

// ---- what dazim_map_tradeoff (tradeoff.hip) shares, declared in map_post_internal.h ----
int dz_mp_period_rows(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, int kmax, int kn, int ncell, int *per, int *span, int *cnt, int *list,
                      std::vector<int> &hcnt) {
  const int64_t m = A->m;
  int *bad = cnt + 2 * kmax;
  DZ_HIP(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_mp_row_period, dim3((unsigned)((m + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, m, A->rowptr, A->col, kn, ncell,
                     per, span, bad);
  DZ_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mp_row_lists, dim3((unsigned)kmax), dim3(MP_TB), 0, ctx->stream, m, m_data, per, cnt, (int *)nullptr);
  DZ_HIP(hipGetLastError());
  hcnt.assign((size_t)2 * kmax + 1, 0);
  DZ_HIP(hipMemcpyAsync(hcnt.data(), cnt, hcnt.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (hcnt[2 * kmax]) return 0;
  hipLaunchKernelGGL(k_mp_row_lists, dim3((unsigned)kmax), dim3(MP_TB), 0, ctx->stream, m, m_data, per, cnt, list);
  DZ_HIP(hipGetLastError());
  return 0;
}

int dz_mp_gram(dazim_ctx *ctx, int ng, int ncell, int kn, int p, int nrow, const int *list, const int *span, const dazim_csr *A, double d2, double *Ad) {
  hipLaunchKernelGGL(k_mp_gram, dim3((unsigned)ng), dim3(64), 0, ctx->stream, ng, ncell, kn, p, nrow, list, span, A->rowptr, A->col, A->val, d2, Ad);
  DZ_HIP(hipGetLastError());
  return 0;
}

void dz_mp_trace(dazim_ctx *ctx, int nb, int ncell, int stride, int off, const double *rd64, float *trace) {
  hipLaunchKernelGGL(k_mp_trace, dim3((unsigned)nb), dim3(MP_TB), 0, ctx->stream, ncell, stride, off, rd64, trace);
}

// dazim_map_posterior and dazim_model_posterior (model_post.hip) share their argument checks, output buffers and row-pass pieces
// (map_post_internal.h).  What differs on the host and stays: the maps keep their matrices in the context's scratch (dz_scratch), the
// model allocates its own for the call (DzOwned); the model finishes the eikonal work (dz_fmm_finish) before dz_join_aux, the maps do
// not; the stats map_post.nb and map_post.mfma are published here only, model_post.n there only.
extern "C" int dazim_map_posterior(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, int nx, int ny, int kmax, int azim, float damp,
                                   float *std_post_u, float *std_noise_u, float *rdiag_u, float *rsum_u, float *width_u, float *leak_u,
                                   int nsel, const int *sel_u, float *rows_u, float *trace_u, int *n_failed) {
  if (!ctx || !A || nx < 3 || ny < 3 || kmax < 1 || !std_post_u || !std_noise_u || !rdiag_u || !rsum_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_map_posterior");
  const int nblk = azim ? 3 : 1;
  const int64_t ncell64 = (int64_t)(nx - 2) * (ny - 2), ng64 = nblk * ncell64;
  int rc;
  if ((rc = dz_post_check_args(ctx, "dazim_map_posterior", A, m_data, A->n == ng64 * kmax, "nblk * kmax * ncell", ng64 * kmax, azim != 0, "azim", leak_u,
                               nullptr, damp, nsel, sel_u, rows_u)))
    return rc;
  const size_t lds = (size_t)ng64 * 8 + (size_t)MP_TB * (8 + MP_EMAX * 8 + 8 + MP_EMAX * 4 + 4);
  if (lds > 160 * 1024) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: %lld unknowns per period do not fit the row pass's LDS", (long long)ng64);
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (int)ncell64, ng = (int)ng64, kn = kmax * ncell, nvx = nx - 2;
  const int64_t m = A->m;
  const size_t no = (size_t)ng * kmax;
  // ---- the workspace, all of it before the first launch ----
  double *Ad, *Cd, *rd64;
  int *per, *span, *cnt, *list, *flags;
  if ((rc = dz_scratch(ctx, "mpost.A", (size_t)ng * ng, &Ad)) || (rc = dz_scratch(ctx, "mpost.C", (size_t)ng * (ng > MP_NB ? ng : MP_NB), &Cd)) ||
      (rc = dz_scratch(ctx, "mpost.rd", (size_t)ng, &rd64)) || (rc = dz_scratch(ctx, "mpost.per", (size_t)m, &per)) || (rc = dz_scratch(ctx, "mpost.span", (size_t)2 * m, &span)) ||
      (rc = dz_scratch(ctx, "mpost.list", (size_t)m, &list)) || (rc = dz_scratch(ctx, "mpost.cnt", (size_t)2 * kmax + 1, &cnt)) ||
      (rc = dz_scratch(ctx, "mpost.flags", (size_t)kmax, &flags)))
    return rc;
  MpOutBufs ob;
  DzBuf<int> sel;
  if ((rc = sel.init(ctx, sel_u, (size_t)nsel, true, false)) ||
      (rc = ob.init(ctx, std_post_u, std_noise_u, rdiag_u, rsum_u, width_u, nullptr, leak_u, rows_u, trace_u, no, (size_t)kmax * nsel * ng, (size_t)nblk * kmax)))
    return rc;
  DZ_HIP(hipFuncSetAttribute((const void *)k_mp_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (a refusal ends the call: no launch)
  if (nsel > 0 && (rc = dz_check_range(ctx, sel.dev, nsel, 0, ng - 1, "dazim_map_posterior: sel"))) return rc;
  // ---- the rows of every period ----
  DZ_HIP(hipMemsetAsync(flags, 0, (size_t)kmax * sizeof(int), ctx->stream));
  std::vector<int> hcnt;
  if ((rc = dz_mp_period_rows(ctx, A, m_data, kmax, kn, ncell, per, span, cnt, list, hcnt))) return rc;
  if (hcnt[2 * kmax] & 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: a row's columns lie in two periods");
  if (hcnt[2 * kmax] & 2) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: a row's columns do not ascend strictly");
  const bool mfma = dz_opt(ctx, "map_post.mfma", 1) != 0;
  const double d2 = (double)damp * (double)damp;
  const MpOut out = ob.dev();
  double sec[5] = {0, 0, 0, 0, 0};
  int off = 0;
  for (int p = 0; p < kmax; p++) {
    const int nrow = hcnt[2 * p], ndat = hcnt[2 * p + 1];
    const int *lp = list + off;
    off += nrow;
    {
      DzTimer t(ctx, "map_post.lap");
      if ((rc = dz_mp_gram(ctx, ng, ncell, kn, p, nrow, lp, span, A, d2, Ad))) return rc;
      t.lap(sec[0]);
    }
    if ((rc = dz_mp_dense(ctx, ng, Ad, Cd, flags + p, mfma, "map_post.lap", sec + 1))) return rc;
    {
      DzTimer t(ctx, "map_post.lap");
      hipLaunchKernelGGL(k_mp_rows, dim3((unsigned)ng), dim3(MP_TB), lds, ctx->stream, ng, ncell, nvx, kn, p, nrow - ndat, lp + ndat, A->rowptr,
                         A->col, A->val, d2, Cd, flags + p, out, nsel, sel.dev, rd64);
      if (ob.tr.dev) dz_mp_trace(ctx, nblk, ncell, kmax, p, rd64, ob.tr.dev);
      DZ_HIP(hipGetLastError());
      t.lap(sec[4]);
    }
  }
  std::vector<int> hflag(kmax);
  DZ_HIP(hipMemcpyAsync(hflag.data(), flags, (size_t)kmax * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = ob.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  int nf = 0;
  for (int p = 0; p < kmax; p++) nf += hflag[p] != 0;
  if (n_failed) *n_failed = nf;
  static const char *names[5] = {"map_post.gram", "map_post.factor", "map_post.inverse", "map_post.c", "map_post.rows"};
  dz_publish_laps(ctx, "map_post.lap", names, sec, 5, "map_posterior");
  ctx->ksec["map_post.nb"] = MP_NB;
  ctx->ksec["map_post.mfma"] = mfma ? 1.0 : 0.0;
  return 0;
}
