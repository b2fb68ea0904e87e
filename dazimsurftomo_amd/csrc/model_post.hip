// model_post.hip -- dazim_model_posterior: posterior std and resolution of the direct 3-D inversion from the
// matrix LSMR is given in an outer iteration, [W G; L], and the damping.  One dense block of n = nblk (nx-2)(ny-2)(nz-1) unknowns:
//   gram     A_n = sum_rows r^T r + damp^2 I, one wavefront per unknown a, driven from the transpose: only the rows that hold a
//   factor, inverse, c   dz_mp_dense (map_post_dense.hip), the kernels of dazim_map_posterior
//   rows     Rm = I - C P entry by entry as a gather over the regularisation entries of column c in the transpose; no row of Rm is
//            stored (but those asked for), LDS holds the partial sums only
// fp64, every sum in a fixed order, no floating-point atomics; the dependencies between the steps are launch order on the context's
// stream.  The two n x n matrices are allocated for the call and released before it returns.
#include <algorithm>
#include <cmath>

#include "map_post_internal.h"

namespace {

constexpr int MO_WPC = 8;   // row-pass workgroups per CU; each keeps its own vector t (one fp64 per regularisation row) in memory

// bad = 1 when a row's columns do not ascend strictly or leave 0..n-1
__global__ __launch_bounds__(MP_TB) void k_mo_check(int64_t m, int n, const int64_t *rowptr, const int *col, int *bad) {
  const int64_t r = (int64_t)blockIdx.x * MP_TB + threadIdx.x;
  if (r >= m) return;
  int prev = -1;
  bool b = false;
  for (int64_t q = rowptr[r]; q < rowptr[r + 1]; q++) {
    const int c = col[q];
    b = b || c <= prev || c >= n;
    prev = c;
  }
  if (b) atomicOr(bad, 1);
}

// regstart[c]: the first entry of column c in the transpose that belongs to a regularisation row (row >= m_data); a column's rows ascend
__global__ __launch_bounds__(MP_TB) void k_mo_regstart(int n, int64_t m_data, const int64_t *colptr, const int *row, int64_t *regstart) {
  const int c = blockIdx.x * MP_TB + threadIdx.x;
  if (c >= n) return;
  int64_t lo = colptr[c], hi = colptr[c + 1];
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)row[mid] < m_data) lo = mid + 1;
    else hi = mid;
  }
  regstart[c] = lo;
}

// row a of A_n (the lower triangle is what the factorisation reads): over the entries (r, v_a) of column a in the transpose, rows
// ascending, A_n(a, c) += v_a r_c for the entries of row r with c <= a (mo_accum_row); then damp^2 on the diagonal.  One wavefront
// per unknown.
__global__ __launch_bounds__(64) void k_mo_gram(int n, const int64_t *colptr, const int *row, const float *tval, const int64_t *rowptr,
                                                const int *col, const float *val, double d2, double *A) {
  const int a = blockIdx.x, t = threadIdx.x;
  double *Aa = A + (size_t)a * n;
  for (int c = t; c < n; c += 64) Aa[c] = 0.0;
  __syncthreads();
  mo_accum_row<false>(a, t, n, colptr[a], colptr[a + 1], row, tval, rowptr, col, val, 1.0, Aa);
  if (t == 0) Aa[a] += d2;
}

// Workgroup g takes the unknowns a = g, g + gridDim.x, ...  For one a: t_l = sum_e C_ae l_e for every regularisation row l (one
// thread per row, ascending e; row a of C is contiguous) into the workgroup's vector tb in memory, then thread t forms
// Rm_ac = delta_ac - sum_l t_l l_c - damp^2 C_ac for c = t, t + MP_TB, ... over column c's regularisation entries in the transpose
// (ascending rows) and adds it to its partial sums; nothing is scattered.
__global__ __launch_bounds__(MP_TB) void k_mo_rows(int n, int ncell, int nvx, int maxvp, int64_t m_data, int64_t mreg, const int64_t *rowptr,
                                                   const int *col, const float *val, const int64_t *colptr, const int64_t *regstart,
                                                   const int *row, const float *tval, double d2, const double *Cm, const int *flag,
                                                   const float *depz, MpOut out, int nsel, const int *sel, double *tbuf, double *rd64) {
  __shared__ double red[MP_TB / 64];
  __shared__ double rdg;
  const int t = threadIdx.x;
  double *tb = tbuf + (size_t)blockIdx.x * (size_t)(mreg > 0 ? mreg : 1);
  const bool failed = *flag != 0;
  for (int a = blockIdx.x; a < n; a += gridDim.x) {
    int nmatch = 0;
    if (out.rows)
      for (int s = 0; s < nsel; s++) nmatch += sel[s] == a;
    if (failed) {
      mp_fill_nan(out, (size_t)a, rd64, a, t, nsel, sel, 0, n);
      continue;
    }
    const double *Ca = Cm + (size_t)a * n;
    for (int64_t l = t; l < mreg; l += MP_TB) {
      double s = 0.0;
      for (int64_t q = rowptr[m_data + l]; q < rowptr[m_data + l + 1]; q++) s += Ca[col[q]] * (double)val[q];
      tb[l] = s;
    }
    __syncthreads();
    const int blk = a / maxvp, ka = (a % maxvp) / ncell, cella = a % ncell, ia = cella % nvx, ja = cella / nvx;
    const double za = depz ? (double)depz[ka] : 0.0;
    MpRowSum<true> sum;
    for (int c = t; c < n; c += MP_TB) {
      double r = c == a ? 1.0 : 0.0;
      const int64_t qe = colptr[c + 1];
      for (int64_t q = regstart[c]; q < qe; q++) r -= tb[(int64_t)row[q] - m_data] * (double)tval[q];
      const double cac = Ca[c];
      r -= d2 * cac;
      const int kc = (c % maxvp) / ncell, cc = c % ncell;
      const double di = (double)(cc % nvx - ia), dj = (double)(cc / nvx - ja), dz = depz ? (double)depz[kc] - za : 0.0;
      sum.add(r, cac, c / maxvp == blk, di * di + dj * dj, dz * dz);
      if (c == a) rdg = r;
      if (nmatch)
        for (int s = 0; s < nsel; s++)
          if (sel[s] == a) out.rows[(size_t)s * n + c] = (float)r;
    }
    sum.reduce(red);
    if (t == 0) sum.write(out, (size_t)a, Ca[a], rdg, rd64, a);
    __syncthreads();   // (tb and rdg belong to the next unknown from here on)
  }
}

}  // namespace

// the row check and regstart, which dazim_model_tradeoff (tradeoff.hip) asks of the same matrix before its own kernels
int dz_mo_check_rows(dazim_ctx *ctx, const dazim_csr *A, int n, int *bad) {
  if (A->m > 0)
    hipLaunchKernelGGL(k_mo_check, dim3((unsigned)((A->m + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, A->m, n, A->rowptr, A->col, bad);
  DZ_HIP(hipGetLastError());
  return 0;
}
int dz_mo_regstart(dazim_ctx *ctx, const dazim_csr *A, int n, int64_t m_data, int64_t *regstart) {
  hipLaunchKernelGGL(k_mo_regstart, dim3((unsigned)((n + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, n, m_data, A->colptr, A->row, regstart);
  DZ_HIP(hipGetLastError());
  return 0;
}

extern "C" int dazim_model_posterior(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, int nx, int ny, int nz, int joint, float damp,
                                     const float *depz_u, float *std_post_u, float *std_noise_u, float *rdiag_u, float *rsum_u,
                                     float *width_h_u, float *width_z_u, float *leak_u, int nsel, const int *sel_u, float *rows_u,
                                     float *trace_u, int *n_failed) {
  if (!ctx || !A || nx < 3 || ny < 3 || nz < 2 || !std_post_u || !std_noise_u || !rdiag_u || !rsum_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_model_posterior");
  const int nblk = joint ? 3 : 1, nlay = nz - 1;
  const int64_t ncell64 = (int64_t)(nx - 2) * (ny - 2), n64 = nblk * ncell64 * nlay;
  int rc;
  if ((rc = dz_post_check_args(ctx, "dazim_model_posterior", A, m_data, A->n == n64 && n64 <= (int64_t)1 << 30, "nblk * (nx-2)(ny-2)(nz-1)", n64, joint != 0,
                               "joint", leak_u, (width_z_u != nullptr) != (depz_u != nullptr) ? "width_z and depz go together" : nullptr, damp, nsel,
                               sel_u, rows_u)))
    return rc;
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_fmm_finish(ctx)) || (rc = dz_join_aux(ctx))) return rc;   // (what differs from dazim_map_posterior's host side: map_post.hip)
  const int ncell = (int)ncell64, n = (int)n64, maxvp = ncell * nlay, nvx = nx - 2;
  const int64_t m = A->m, mreg = m - m_data;
  // ---- the workspace: refused before the first launch when the card cannot hold it ----
  const int ngrid = (int)std::min<int64_t>(n, (int64_t)MO_WPC * ctx->num_cu);
  const size_t bA = (size_t)n * n * 8, bC = (size_t)n * (n > MP_NB ? n : MP_NB) * 8, bT = (size_t)ngrid * (size_t)(mreg > 0 ? mreg : 1) * 8;
  const size_t bTr = A->colptr ? 0 : (size_t)(n + 1) * 8 + (size_t)(A->nnz > 0 ? A->nnz : 1) * 12 * 3;   // (the transpose and its sort)
  if ((rc = dz_need_device_bytes(ctx, bA + bC + bT + bTr + ((size_t)64 << 20), "dazim_model_posterior", (long long)n64, "unknowns"))) return rc;
  if (!A->colptr && (rc = dz_build_transpose(ctx, const_cast<dazim_csr *>(A)))) return rc;
  DzOwned big;
  DZ_HIP(dz_malloc_retry(ctx, &big.p[0], bA));
  DZ_HIP(dz_malloc_retry(ctx, &big.p[1], bC));
  DZ_HIP(dz_malloc_retry(ctx, &big.p[2], bT));
  double *Ad = (double *)big.p[0], *Cd = (double *)big.p[1], *tbuf = (double *)big.p[2], *rd64;
  int64_t *regstart;
  int *flags;
  if ((rc = dz_scratch(ctx, "mopost.rd", (size_t)n, &rd64)) || (rc = dz_scratch(ctx, "mopost.reg", (size_t)n, &regstart)) ||
      (rc = dz_scratch(ctx, "mopost.flags", (size_t)2, &flags)))
    return rc;
  MpOutBufs ob;
  DzBuf<float> dz;
  DzBuf<int> sel;
  if ((rc = sel.init(ctx, sel_u, (size_t)nsel, true, false)) || (rc = dz.init(ctx, depz_u, depz_u ? (size_t)nlay : 0, true, false)) ||
      (rc = ob.init(ctx, std_post_u, std_noise_u, rdiag_u, rsum_u, width_h_u, width_z_u, leak_u, rows_u, trace_u, (size_t)n, (size_t)nsel * n, (size_t)nblk * nlay)))
    return rc;
  if (nsel > 0 && (rc = dz_check_range(ctx, sel.dev, nsel, 0, n - 1, "dazim_model_posterior: sel"))) return rc;
  int hflag[2] = {0, 0};
  DZ_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int), ctx->stream));
  if ((rc = dz_mo_check_rows(ctx, A, n, flags + 1))) return rc;
  DZ_HIP(hipMemcpyAsync(hflag, flags, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (hflag[1]) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_posterior: a row's columns do not ascend strictly inside 0..n-1");
  const bool mfma = dz_opt(ctx, "map_post.mfma", 1) != 0;
  const double d2 = (double)damp * (double)damp;
  const MpOut out = ob.dev();
  double sec[5] = {0, 0, 0, 0, 0};
  {
    DzTimer t(ctx, "model_post.lap");
    if ((rc = dz_mo_regstart(ctx, A, n, m_data, regstart))) return rc;
    hipLaunchKernelGGL(k_mo_gram, dim3((unsigned)n), dim3(64), 0, ctx->stream, n, A->colptr, A->row, A->tval, A->rowptr, A->col, A->val, d2, Ad);
    DZ_HIP(hipGetLastError());
    t.lap(sec[0]);
  }
  if ((rc = dz_mp_dense(ctx, n, Ad, Cd, flags, mfma, "model_post.lap", sec + 1))) return rc;
  {
    DzTimer t(ctx, "model_post.lap");
    hipLaunchKernelGGL(k_mo_rows, dim3((unsigned)ngrid), dim3(MP_TB), 0, ctx->stream, n, ncell, nvx, maxvp, m_data, mreg, A->rowptr, A->col, A->val,
                       A->colptr, regstart, A->row, A->tval, d2, Cd, flags, dz.dev, out, nsel, sel.dev, tbuf, rd64);
    if (ob.tr.dev) dz_mp_trace(ctx, nblk * nlay, ncell, 1, 0, rd64, ob.tr.dev);
    DZ_HIP(hipGetLastError());
    t.lap(sec[4]);
  }
  DZ_HIP(hipMemcpyAsync(hflag, flags, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = ob.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_failed) *n_failed = hflag[0] != 0;
  static const char *names[5] = {"model_post.gram", "model_post.factor", "model_post.inverse", "model_post.c", "model_post.rows"};
  dz_publish_laps(ctx, "model_post.lap", names, sec, 5, "model_posterior");
  ctx->ksec["model_post.n"] = (double)n;
  return 0;
}
