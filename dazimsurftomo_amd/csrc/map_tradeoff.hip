// map_tradeoff.hip -- dazim_map_tradeoff: a sweep over regularisation strengths of the per-period phase-velocity maps' linearised step
// (DESIGN.md section 12.2), on the exact fp64 dense normal matrix of dazim_map_posterior.  The normal matrix is block diagonal by period;
// per period p of n_g = nblk ncell unknowns (local index a = blk ncell + cell):
//   once     D_p = sum over the period's data rows of r^T r (k_mp_gram with d^2 = 0), mirrored to both triangles; g_p = sum r^T b_r
//   point k  combine   W = D_p + sum_b scale[k][b]^2 R_pb + damp[k]^2 I: D_p's row, then the period's regularisation rows, ascending
//            factor    dz_mp_factor (map_post_dense.hip) on W; D_p is never factored
//            solve     R y = g_p, R^T x = y (dz_mt_solve, model_tradeoff.hip)
//            sums      log det, |G_p x - b_p|^2, |L_pb x|^2 per block, |x|^2
//            inverse   (want_dof) dz_mp_inverse_c, then sum_c C_ac D_ac per row and the rows of a block
//            evidence  (want_evidence) W = P alone, factored again for log det P
// fp64, every sum in a fixed order that depends on the problem alone, no floating-point atomics; the dependencies between the steps
// are launch order on the context's stream.  The n_g x n_g matrices are allocated for the call and released on every way out.
#include <algorithm>
#include <cmath>
#include <vector>

#include "map_post_internal.h"

namespace {

constexpr int MPT_RG = 16;   // rows per wavefront in the row sums

struct MptScale {
  double s2[3];
};

// bad |= 1 when a regularisation row has entries in two blocks (its columns ascend: the first and the last decide)
__global__ __launch_bounds__(MP_TB) void k_mpt_block(int64_t m_data, int64_t mreg, int kn, const int64_t *rowptr, const int *col, int *bad) {
  const int64_t l = (int64_t)blockIdx.x * MP_TB + threadIdx.x;
  if (l >= mreg) return;
  const int64_t b = rowptr[m_data + l], e = rowptr[m_data + l + 1];
  if (e > b && col[b] / kn != col[e - 1] / kn) atomicOr(bad, 1);
}

// row a of the work matrix, c <= a: src's row (D_p; nullptr: zero, for P alone), then the period's regularisation rows, ascending,
// each product times the squared scale of a's block (the block of every row that holds a), then damp^2 on the diagonal.  At scale 1
// these are k_mp_gram's numbers, added in k_mp_gram's order.
__global__ __launch_bounds__(64) void k_mpt_combine(int ng, int ncell, int kn, int p, int nreg, const int *reglist, const int *span,
                                                    const int64_t *rowptr, const int *col, const float *val, const double *src, MptScale sc,
                                                    double d2, double *W) {
  const int a = blockIdx.x, t = threadIdx.x;
  double *Wa = W + (size_t)a * ng;
  const double *Sa = src ? src + (size_t)a * ng : nullptr;
  for (int c = t; c <= a; c += 64) Wa[c] = Sa ? Sa[c] : 0.0;
  __syncthreads();
  mp_accum_rows<true>(a, t, ncell, kn, p, nreg, reglist, span, rowptr, col, val, sc.s2[a / ncell], Wa);
  if (t == 0) Wa[a] += d2;
}

// g[a] = sum over the period's data rows r that hold column a, ascending, of r_a b_r: one wavefront per a, the rows found as
// mp_accum_rows finds them; every lane carries the same sum
__global__ __launch_bounds__(64) void k_mpt_rhs(int ncell, int kn, int p, int ndat, const int *list, const int *span, const int64_t *rowptr,
                                                const int *col, const float *val, const float *b, double *g) {
  const int a = blockIdx.x, t = threadIdx.x, cell_a = a % ncell;
  const int ga = (a / ncell) * kn + p * ncell + a % ncell;
  double s = 0.0;
  for (int i0 = 0; i0 < ndat; i0 += 64) {
    long long mb = 0, me = 0;
    int r = 0;
    bool near = false;
    if (i0 + t < ndat) {
      r = list[i0 + t];
      mb = rowptr[r];
      me = rowptr[r + 1];
      near = span[2 * (size_t)r] <= cell_a && cell_a <= span[2 * (size_t)r + 1];
    }
    for (unsigned long long cand = __ballot(near); cand; cand &= cand - 1ull) {   // ascending rows
      const int k = __ffsll((long long)cand) - 1;
      const long long qb = __shfl(mb, k), qe = __shfl(me, k);
      const int rk = __shfl(r, k);
      float va = 0.0f;
      bool hit = false;
      for (long long q = qb + t; q < qe; q += 64)
        if (col[q] == ga) {
          va = val[q];
          hit = true;
        }
      const unsigned long long h = __ballot(hit);
      if (!h) continue;
      s += (double)__shfl(va, __ffsll((long long)h) - 1) * (double)b[rk];
    }
  }
  if (t == 0) g[a] = s;
}

// wavefront w takes the rows list[w MPT_RG ..] of one period: t = sum_q val_q x[local col_q] (lane l the entries l, l + 64, ...;
// butterfly), minus b_r for the data rows; t^2 goes to the slot of the row's block (data rows: slot 0), in the order of the list.
// part [groups][3].
template <bool REG>
__global__ __launch_bounds__(MP_TB) void k_mpt_rows(int nrows, const int *list, int ncell, int kn, const int64_t *rowptr, const int *col,
                                                    const float *val, const double *x, const float *b, double *part) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * (MP_TB / 64) + (threadIdx.x >> 6), ngroup = (nrows + MPT_RG - 1) / MPT_RG;
  if (g >= ngroup) return;
  double acc[3] = {0.0, 0.0, 0.0};
  const int le = min((g + 1) * MPT_RG, nrows);
  for (int l = g * MPT_RG; l < le; l++) {
    const int r = list[l];
    const int64_t qb = rowptr[r], qe = rowptr[r + 1];
    double s = 0.0;
    for (int64_t q = qb + lane; q < qe; q += 64) s += (double)val[q] * x[mp_local(col[q], kn, ncell)];
    s = wave_sum(s);
    if (REG) {
      acc[col[qb] / kn] += s * s;   // (a row of the list has entries)
    } else {
      s -= (double)b[r];
      acc[0] += s * s;
    }
  }
  if (lane == 0)
    for (int k = 0; k < 3; k++) part[(size_t)g * 3 + k] = acc[k];
}

struct MptOut {
  double *chi2, *reg2, *xnorm2, *logdet_a, *logdet_p, *dof, *gcv, *logev;
};
enum { MPT_CHI2 = 0, MPT_REG2 = 1, MPT_XN = 4, MPT_LDA = 5, MPT_LDP = 6, MPT_DOF = 7, MPT_NSC = 10 };

// the outputs of point k, period p (slot kp = k kmax + p) from its sums sc[MPT_NSC]; flag[0]: A could not be factored (every output
// NaN), flag[1]: P could not
__global__ void k_mpt_final(int kp, int nblk, int64_t mp, MptScale s, double d2, int want_dof, int want_ev, const int *flag, const double *sc,
                            MptOut o) {
  const double nan = __builtin_nan("");
  const bool failed = flag[0] != 0;
  double J = d2 * sc[MPT_XN], dofs = 0.0;
  for (int b = 0; b < nblk; b++) {
    J += s.s2[b] * sc[MPT_REG2 + b];
    dofs += sc[MPT_DOF + b];
    o.reg2[kp * nblk + b] = failed ? nan : sc[MPT_REG2 + b];
    if (want_dof && o.dof) o.dof[kp * nblk + b] = failed ? nan : sc[MPT_DOF + b];
  }
  o.chi2[kp] = failed ? nan : sc[MPT_CHI2];
  o.xnorm2[kp] = failed ? nan : sc[MPT_XN];
  o.logdet_a[kp] = failed ? nan : sc[MPT_LDA];
  if (want_dof && o.gcv) {
    const double den = (double)mp - dofs;
    o.gcv[kp] = failed ? nan : (double)mp * sc[MPT_CHI2] / (den * den);
  }
  if (want_ev) {
    const double ldp = (failed || flag[1] != 0) ? nan : sc[MPT_LDP];
    if (o.logdet_p) o.logdet_p[kp] = ldp;
    if (o.logev) o.logev[kp] = failed ? nan : -0.5 * (sc[MPT_CHI2] + J) + 0.5 * ldp - 0.5 * sc[MPT_LDA] - 0.5 * (double)mp * log(6.283185307179586476925);
  }
}

// the period's solution, rounded once, into the layout of dm: out[blk kn + p ncell + cell]
__global__ __launch_bounds__(MP_TB) void k_mpt_xout(int ng, int ncell, int kn, int p, const double *x, const int *flag, float *out) {
  const int a = blockIdx.x * MP_TB + threadIdx.x;
  if (a < ng) out[(size_t)(a / ncell) * kn + (size_t)p * ncell + a % ncell] = *flag ? nanf("") : (float)x[a];
}

struct MptBig {   // the call's own allocations: released on every way out
  void *p[3] = {nullptr, nullptr, nullptr};
  ~MptBig() {
    for (void *q : p)
      if (q) (void)hipFree(q);
  }
};

}  // namespace

extern "C" int dazim_map_tradeoff(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, const float *b_u, int nx, int ny, int kmax, int azim, int K,
                                  const float *scale, const float *damp, int want_dof, int want_evidence, int64_t *mdata_p_u, double *chi2_u,
                                  double *reg2_u, double *xnorm2_u, double *logdet_a_u, double *logdet_p_u, double *dof_u, double *gcv_u,
                                  double *logev_u, float *x_u, int *n_failed) {
  if (!ctx || !A || nx < 3 || ny < 3 || kmax < 1 || !scale || !damp || !chi2_u || !reg2_u || !xnorm2_u || !logdet_a_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_map_tradeoff");
  if (dz_is_device_ptr(scale) || dz_is_device_ptr(damp)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: scale and damp are host arrays");
  if (K < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: K %d < 1", K);
  if (!b_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: no right-hand side b");
  if (m_data < 0 || m_data > A->m)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: m_data %lld outside 0..%lld", (long long)m_data, (long long)A->m);
  const int nblk = azim ? 3 : 1;
  const int64_t ncell64 = (int64_t)(nx - 2) * (ny - 2), ng64 = nblk * ncell64;
  if (A->n != ng64 * kmax)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: n %lld is not nblk * kmax * ncell = %lld", (long long)A->n, (long long)(ng64 * kmax));
  if (!want_dof && (dof_u || gcv_u)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: dof or gcv without want_dof");
  if (!want_evidence && (logdet_p_u || logev_u)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: logdet_p or logev without want_evidence");
  for (int k = 0; k < K; k++) {
    if (!(damp[k] >= 0.0f) || !std::isfinite(damp[k])) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: damp[%d] negative or not finite", k);
    for (int b = 0; b < nblk; b++)
      if (!(scale[k * nblk + b] >= 0.0f) || !std::isfinite(scale[k * nblk + b]))
        return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: scale[%d][%d] negative or not finite", k, b);
  }
  DZ_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (int)ncell64, ng = (int)ng64, kn = kmax * ncell;
  const int64_t m = A->m, mreg = m - m_data, n = A->n;
  // ---- the workspace: refused before the first launch when the card cannot hold it ----
  const size_t bA = (size_t)ng * ng * 8, bC = want_dof ? (size_t)ng * (ng > MP_NB ? ng : MP_NB) * 8 : 0;
  const size_t need = 2 * bA + bC + (size_t)m * 16 + ((size_t)64 << 20);
  size_t fre = 0, tot = 0;
  DZ_HIP(hipMemGetInfo(&fre, &tot));
  if (need > fre) {
    (void)dz_trim_caches(ctx);
    DZ_HIP(hipMemGetInfo(&fre, &tot));
  }
  if (need > fre)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: %lld unknowns per period need %.1f GiB of device memory, %.1f GiB are free",
                   (long long)ng64, (double)need / 1073741824.0, (double)fre / 1073741824.0);
  MptBig big;
  DZ_HIP(dz_malloc_retry(ctx, &big.p[0], bA));
  DZ_HIP(dz_malloc_retry(ctx, &big.p[1], bA));
  if (want_dof) DZ_HIP(dz_malloc_retry(ctx, &big.p[2], bC));
  double *Dd = (double *)big.p[0], *Wd = (double *)big.p[1], *Cd = (double *)big.p[2];
  double *g, *y, *part, *rowdot, *sc;
  int *per, *span, *cnt, *list, *flags;
  const size_t kk = (size_t)K * kmax;
  if ((rc = dz_scratch(ctx, "mptrade.g", (size_t)ng, &g)) || (rc = dz_scratch(ctx, "mptrade.y", (size_t)ng, &y)) ||
      (rc = dz_scratch(ctx, "mptrade.part", (size_t)(m / MPT_RG + 2) * 3, &part)) || (rc = dz_scratch(ctx, "mptrade.rowdot", (size_t)ng, &rowdot)) ||
      (rc = dz_scratch(ctx, "mptrade.sc", (size_t)MPT_NSC, &sc)) || (rc = dz_scratch(ctx, "mptrade.per", (size_t)std::max<int64_t>(m, 1), &per)) ||
      (rc = dz_scratch(ctx, "mptrade.span", (size_t)2 * std::max<int64_t>(m, 1), &span)) ||
      (rc = dz_scratch(ctx, "mptrade.list", (size_t)std::max<int64_t>(m, 1), &list)) || (rc = dz_scratch(ctx, "mptrade.cnt", (size_t)2 * kmax + 1, &cnt)) ||
      (rc = dz_scratch(ctx, "mptrade.flags", 2 * kk + 1, &flags)))
    return rc;
  DzBuf<float> bb, xo;
  DzBuf<double> o_chi, o_reg, o_xn, o_lda, o_ldp, o_dof, o_gcv, o_lev;
  if ((rc = bb.init(ctx, b_u, (size_t)m_data, true, false)) || (rc = xo.init(ctx, x_u, x_u ? (size_t)K * n : 0, false, true)) ||
      (rc = o_chi.init(ctx, chi2_u, kk, false, true)) ||
      (rc = o_reg.init(ctx, reg2_u, kk * nblk, false, true)) || (rc = o_xn.init(ctx, xnorm2_u, kk, false, true)) ||
      (rc = o_lda.init(ctx, logdet_a_u, kk, false, true)) || (rc = o_ldp.init(ctx, logdet_p_u, logdet_p_u ? kk : 0, false, true)) ||
      (rc = o_dof.init(ctx, dof_u, dof_u ? kk * nblk : 0, false, true)) || (rc = o_gcv.init(ctx, gcv_u, gcv_u ? kk : 0, false, true)) ||
      (rc = o_lev.init(ctx, logev_u, logev_u ? kk : 0, false, true)))
    return rc;
  // ---- the rows of every period, and the block of every regularisation row ----
  std::vector<int> hflag(2 * kk + 1, 0), hcnt;
  int *bad = flags + 2 * kk;
  DZ_HIP(hipMemsetAsync(flags, 0, (2 * kk + 1) * sizeof(int), ctx->stream));
  if (mreg > 0)
    hipLaunchKernelGGL(k_mpt_block, dim3((unsigned)((mreg + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, m_data, mreg, kn, A->rowptr, A->col, bad);
  DZ_HIP(hipGetLastError());
  DZ_HIP(hipMemcpyAsync(hflag.data() + 2 * kk, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = dz_mp_period_rows(ctx, A, m_data, kmax, kn, ncell, per, span, cnt, list, hcnt))) return rc;   // (synchronises)
  if (hcnt[2 * kmax] & 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: a row's columns lie in two periods");
  if (hcnt[2 * kmax] & 2) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: a row's columns do not ascend strictly");
  if (hflag[2 * kk]) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: a regularisation row spans two blocks");
  const bool mfma = dz_opt(ctx, "map_post.mfma", 1) != 0;
  const char *lapname = "map_trade.lap";
  double sec[4] = {0, 0, 0, 0};   // gram, factor, solve, inverse
  auto lap = [&](int which, DzTimer &t) {
    t.stop();
    sec[which] += ctx->ksec[lapname];
  };
  const MptOut out = {o_chi.dev, o_reg.dev, o_xn.dev, o_lda.dev, o_ldp.dev, o_dof.dev, o_gcv.dev, o_lev.dev};
  std::vector<int64_t> hmp((size_t)kmax);
  DZ_HIP(hipMemsetAsync(Wd, 0, bA, ctx->stream));   // (the upper triangle of the work matrix is never written or read)
  int off = 0, grams = 0;
  for (int p = 0; p < kmax; p++) {
    const int nrow = hcnt[2 * p], ndat = hcnt[2 * p + 1], nreg = nrow - ndat;
    const int *lp = list + off, *lr = lp + ndat;
    off += nrow;
    hmp[p] = ndat;
    const int gdata = (ndat + MPT_RG - 1) / MPT_RG, greg = (nreg + MPT_RG - 1) / MPT_RG;
    {
      DzTimer t(ctx, lapname);
      if ((rc = dz_mp_gram(ctx, ng, ncell, kn, p, ndat, lp, span, A, 0.0, Dd)) || (rc = dz_mt_mirror(ctx, ng, Dd))) return rc;
      grams++;
      hipLaunchKernelGGL(k_mpt_rhs, dim3((unsigned)ng), dim3(64), 0, ctx->stream, ncell, kn, p, ndat, lp, span, A->rowptr, A->col, A->val, bb.dev, g);
      DZ_HIP(hipGetLastError());
      lap(0, t);
    }
    for (int k = 0; k < K; k++) {
      MptScale s;
      for (int b = 0; b < 3; b++) s.s2[b] = b < nblk ? (double)scale[k * nblk + b] * (double)scale[k * nblk + b] : 0.0;
      const double d2 = (double)damp[k] * (double)damp[k];
      const int kp = k * kmax + p;
      int *fl = flags + 2 * (size_t)kp;
      {
        DzTimer t(ctx, lapname);
        hipLaunchKernelGGL(k_mpt_combine, dim3((unsigned)ng), dim3(64), 0, ctx->stream, ng, ncell, kn, p, nreg, lr, span, A->rowptr, A->col, A->val,
                           (const double *)Dd, s, d2, Wd);
        DZ_HIP(hipGetLastError());
        lap(1, t);
      }
      if ((rc = dz_mp_factor(ctx, ng, Wd, fl, mfma, lapname, sec + 1))) return rc;
      {
        DzTimer t(ctx, lapname);
        DZ_HIP(hipMemsetAsync(sc, 0, MPT_NSC * sizeof(double), ctx->stream));
        DZ_HIP(hipMemcpyAsync(y, g, (size_t)ng * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        if ((rc = dz_mt_solve(ctx, ng, Wd, y)) || (rc = dz_mt_logdet_norm(ctx, ng, Wd, y, sc + MPT_LDA, sc + MPT_XN))) return rc;
        if (gdata > 0) {
          hipLaunchKernelGGL(k_mpt_rows<false>, dim3((unsigned)((gdata + MP_TB / 64 - 1) / (MP_TB / 64))), dim3(MP_TB), 0, ctx->stream, ndat, lp, ncell, kn,
                             A->rowptr, A->col, A->val, (const double *)y, (const float *)bb.dev, part);
          if ((rc = dz_mt_sum(ctx, 1, gdata, 3, 1, part, sc + MPT_CHI2))) return rc;
        }
        if (greg > 0) {
          hipLaunchKernelGGL(k_mpt_rows<true>, dim3((unsigned)((greg + MP_TB / 64 - 1) / (MP_TB / 64))), dim3(MP_TB), 0, ctx->stream, nreg, lr, ncell, kn,
                             A->rowptr, A->col, A->val, (const double *)y, (const float *)nullptr, part);
          if ((rc = dz_mt_sum(ctx, nblk, greg, 3, 1, part, sc + MPT_REG2))) return rc;
        }
        if (xo.dev)
          hipLaunchKernelGGL(k_mpt_xout, dim3((unsigned)((ng + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, ng, ncell, kn, p, (const double *)y,
                             (const int *)fl, xo.dev + (size_t)k * n);
        DZ_HIP(hipGetLastError());
        lap(2, t);
      }
      if (want_dof) {
        double s3[3] = {0, 0, 0};
        if ((rc = dz_mp_inverse_c(ctx, ng, Wd, Cd, mfma, lapname, s3))) return rc;
        DzTimer t(ctx, lapname);
        if ((rc = dz_mt_rowdot(ctx, ng, Cd, Dd, rowdot)) || (rc = dz_mt_sum(ctx, nblk, ncell, 1, ncell, rowdot, sc + MPT_DOF))) return rc;
        lap(3, t);
        sec[3] += s3[1] + s3[2];
      }
      if (want_evidence) {
        {
          DzTimer t(ctx, lapname);
          hipLaunchKernelGGL(k_mpt_combine, dim3((unsigned)ng), dim3(64), 0, ctx->stream, ng, ncell, kn, p, nreg, lr, span, A->rowptr, A->col, A->val,
                             (const double *)nullptr, s, d2, Wd);
          DZ_HIP(hipGetLastError());
          lap(1, t);
        }
        if ((rc = dz_mp_factor(ctx, ng, Wd, fl + 1, mfma, lapname, sec + 1))) return rc;
        DzTimer t(ctx, lapname);
        if ((rc = dz_mt_logdet_norm(ctx, ng, Wd, nullptr, sc + MPT_LDP, nullptr))) return rc;
        lap(1, t);
      }
      hipLaunchKernelGGL(k_mpt_final, dim3(1), dim3(1), 0, ctx->stream, kp, nblk, (int64_t)ndat, s, d2, want_dof, want_evidence, (const int *)fl,
                         (const double *)sc, out);
      DZ_HIP(hipGetLastError());
    }
  }
  const bool mp_dev = mdata_p_u && dz_is_device_ptr(mdata_p_u);
  if (mp_dev) DZ_HIP(hipMemcpyAsync(mdata_p_u, hmp.data(), (size_t)kmax * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync(hflag.data(), flags, 2 * kk * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = xo.finish()) || (rc = o_chi.finish()) || (rc = o_reg.finish()) || (rc = o_xn.finish()) || (rc = o_lda.finish()) || (rc = o_ldp.finish()) ||
      (rc = o_dof.finish()) || (rc = o_gcv.finish()) || (rc = o_lev.finish()))
    return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (mdata_p_u && !mp_dev)
    for (int p = 0; p < kmax; p++) mdata_p_u[p] = hmp[p];
  if (n_failed)
    for (size_t i = 0; i < kk; i++) n_failed[i] = hflag[2 * i] != 0;
  ctx->ksec.erase(lapname);
  static const char *names[4] = {"map_trade.gram", "map_trade.factor", "map_trade.solve", "map_trade.inverse"};
  double total = 0.0;
  for (int i = 0; i < 4; i++) {
    ctx->ksec[names[i]] = sec[i];
    total += sec[i];
  }
  ctx->ksec["map_tradeoff"] = total;
  ctx->ksec["map_trade.points"] = (double)K;
  ctx->ksec["map_trade.ng"] = (double)ng;
  ctx->ksec["map_trade.grams"] = (double)grams;
  return 0;
}

// The criteria of the whole block-diagonal system from dazim_map_tradeoff's per-period arrays (host only): every total the sum over
// the periods in ascending p (reg2sum_t and dof_t over p and then blk), gcv_t = M chi2_t / (M - dof_t)^2 with M = sum_p m_p.
extern "C" int dazim_map_tradeoff_total(int K, int kmax, int nblk, const int64_t *mdata_p, const double *chi2, const double *reg2, const double *dof,
                                        const double *logev, double *chi2_t, double *reg2sum_t, double *dof_t, double *gcv_t, double *logev_t) {
  if (K < 1 || kmax < 1 || nblk < 1 || !mdata_p || !chi2 || !reg2 || !chi2_t || !reg2sum_t) return DAZIM_E_BAD_ARG;
  if ((!dof && (dof_t || gcv_t)) || (!logev && logev_t)) return DAZIM_E_BAD_ARG;
  double M = 0.0;
  for (int p = 0; p < kmax; p++) M += (double)mdata_p[p];
  for (int k = 0; k < K; k++) {
    double c = 0.0, r = 0.0, d = 0.0, e = 0.0;
    for (int p = 0; p < kmax; p++) {
      const size_t kp = (size_t)k * kmax + p;
      c += chi2[kp];
      if (logev) e += logev[kp];
      for (int b = 0; b < nblk; b++) {
        r += reg2[kp * nblk + b];
        if (dof) d += dof[kp * nblk + b];
      }
    }
    chi2_t[k] = c;
    reg2sum_t[k] = r;
    if (dof_t) dof_t[k] = d;
    if (gcv_t) gcv_t[k] = M * c / ((M - d) * (M - d));
    if (logev_t) logev_t[k] = e;
  }
  return 0;
}
