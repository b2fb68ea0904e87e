// column.hip -- the second step of the two-step method: from per-period maps to a depth model, cell by cell.
//
// dazim_vs_kernels: the dc/dVs table the 3-D rows multiply (k_row_kernels of rays.hip, through the same dz_row_kernel).
// dazim_column_lsq: one small regularised dense least-squares problem per inner map cell, all cells in one launch: one wavefront
// per cell builds its normal matrix (at most 63 x 63) in LDS, factors it by Cholesky and solves, all in fp64.  The launch is bound
// by latency (a few MB of kernel table in all), so it stays this plain.  Every sum runs in a fixed order: the same inputs give the
// same bits, whether they come from the host or the device.
// dazim_column_resolution: posterior covariance and resolution matrix of that problem from the same factor, in the same launch shape.
#include "dazim_internal.h"

#include <cmath>

namespace {

constexpr int CL_MAXLAY = 63, CL_MAXPER = 60, CL_WAVE = 64, CL_STATS_TB = 256;

__global__ void k_vs_kernels(long n, int kmax, long ncol, const float *__restrict__ vels, const double *__restrict__ svs,
                             const double *__restrict__ svp, const double *__restrict__ srho, double *__restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // (layer, period, column), as k_row_kernels
  if (i >= n) return;
  const long k = i / (kmax * ncol), c = i % ncol;
  out[i] = dz_row_kernel(vels[k * ncol + c], svs[i], svp[i], srho[i]);
}

// One wavefront per inner cell (j, i) of the map, column (j+1)*nx + i+1 of the kernel table:
//   min ||diag(w)(K x - r)||^2 + s2 ||L x||^2 + d2 ||x||^2  for each of the nrhs right-hand sides r,
// by the normal equations (K^T W^2 K + s2 L^T L + d2 I) x = K^T W^2 r and their Cholesky factor: dz_column_solve of
// dazim_internal.h, which k_mc_aniso of column_mc.hip calls too.
// LDS: A [n][n] (the normal matrix, then its factor in the lower triangle), K [kmax][n], w^2 [kmax], w^2 r [nrhs][kmax],
// b [nrhs][n] (right-hand sides, then solutions): at most 64 440 bytes for n = 63, kmax = 60, nrhs = 2.
template <typename KT>
__global__ __launch_bounds__(CL_WAVE) void k_column_lsq(int nx, int ny, int n, int kmax, const KT *__restrict__ kern, int nrhs,
                                                        const float *__restrict__ rhs, const float *__restrict__ wdat, double s2,
                                                        double d2, float *__restrict__ x, int *__restrict__ n_empty,
                                                        double *__restrict__ part) {
  extern __shared__ double sm[];
  double *A = sm;
  double *K = A + n * n;
  double *w2 = K + kmax * n;
  double *wr = w2 + kmax;
  double *b = wr + nrhs * kmax;
  const int t = threadIdx.x;
  const int nvx = nx - 2, ncell = nvx * (ny - 2);
  const int cell = blockIdx.x;
  const int j = cell / nvx, i = cell - j * nvx;
  const long ncol = (long)nx * ny, col = (long)(j + 1) * nx + (i + 1);

  bool data = false;
  if (t < kmax) {
    const float w = wdat ? wdat[(long)t * ncell + cell] : 1.0f;
    data = w != 0.0f;
    const double ww = (double)w * (double)w;
    w2[t] = ww;
    for (int r = 0; r < nrhs; r++) wr[r * kmax + t] = data ? ww * (double)rhs[((long)r * kmax + t) * ncell + cell] : 0.0;
  }
  if (!__any(data)) {   // no data in this cell: x = 0 exactly
    for (int q = t; q < nrhs * n; q += CL_WAVE) x[(long)q * ncell + cell] = 0.0f;
    if (part && t < kmax)
      for (int r = 0; r < nrhs; r++) {
        const long o = ((long)(r * kmax + t) * ncell + cell) * 2;
        part[o] = 0.0;
        part[o + 1] = 0.0;
      }
    if (t == 0) atomicAdd(n_empty, 1);
    return;
  }
  for (int q = t; q < n * kmax; q += CL_WAVE) {   // q = l*kmax + p, the table's own order
    const int l = q / kmax, p = q - l * kmax;
    K[p * n + l] = (double)kern[(long)q * ncol + col];
  }
  __syncthreads();
  dz_column_solve(t, n, kmax, nrhs, A, K, w2, wr, b, s2, d2);
  for (int q = t; q < nrhs * n; q += CL_WAVE) x[(long)q * ncell + cell] = (float)b[q];
  if (part && t < kmax)                           // r^2 and (r - K x)^2 of this cell, 0 where w = 0
    for (int r = 0; r < nrhs; r++) {
      double rr = 0.0, ee = 0.0;
      if (w2[t] != 0.0) {
        const double rv = (double)rhs[((long)r * kmax + t) * ncell + cell];
        double kx = 0.0;
        for (int l = 0; l < n; l++) kx += K[t * n + l] * b[r * n + l];
        rr = rv * rv;
        ee = (rv - kx) * (rv - kx);
      }
      const long o = ((long)(r * kmax + t) * ncell + cell) * 2;
      part[o] = rr;
      part[o + 1] = ee;
    }
}

// per (right-hand side, period): RMS over the cells with w != 0 of r and of r - K x, from the cells' partial sums (fixed order)
__global__ __launch_bounds__(CL_STATS_TB) void k_column_stats(int ncell, int kmax, const float *__restrict__ wdat,
                                                              const double *__restrict__ part, float *__restrict__ out) {
  __shared__ double s[3][CL_STATS_TB];
  const int rp = blockIdx.x, p = rp % kmax, t = threadIdx.x;
  double a = 0.0, e = 0.0, cnt = 0.0;
  for (int c = t; c < ncell; c += CL_STATS_TB) {
    const float w = wdat ? wdat[(long)p * ncell + c] : 1.0f;
    if (w == 0.0f) continue;
    const long o = ((long)rp * ncell + c) * 2;
    a += part[o];
    e += part[o + 1];
    cnt += 1.0;
  }
  s[0][t] = a;
  s[1][t] = e;
  s[2][t] = cnt;
  __syncthreads();
  for (int h = CL_STATS_TB / 2; h > 0; h >>= 1) {
    if (t < h)
      for (int q = 0; q < 3; q++) s[q][t] += s[q][t + h];
    __syncthreads();
  }
  if (t == 0) {
    out[rp * 2] = s[2][0] > 0.0 ? (float)sqrt(s[0][0] / s[2][0]) : 0.0f;
    out[rp * 2 + 1] = s[2][0] > 0.0 ? (float)sqrt(s[1][0] / s[2][0]) : 0.0f;
  }
}

// Posterior covariance and resolution of k_column_lsq's problem, one 64-lane workgroup per inner cell, lane = knot a.  With
// A = K^T W^2 K + P, P = s2 L^T L + d2 I, and A = R R^T from dz_column_solve (nrhs = 0: it builds and factors A and touches neither
// wr nor b): M = R^-1 by dz_column_inverse_factor (column k in row k of A's strict upper triangle, then 1 / R_kk on the diagonal),
// C = A^-1 = M^T M, Rm = I - C P.  Lane a forms row a of C, C_ac = sum_{i >= max(a, c)} M_ia M_ic in ascending i (C_aa is
// dz_column_inverse_factor's sum), keeps it in its own row of Cm and walks it once: Rm_ac from the five entries C_ae, |e - c| <= 2,
// that the pentadiagonal P reaches, and with it the row sum, the spread about z_a and, where asked, the row itself; (Rm C)_aa comes
// from the same row as sum_p w_p^2 (sum_c C_ac K_pc)^2.  Barriers stand where a lane reads another lane's row of A.
// LDS: A [n][n], K [kmax][n] (at the end the lanes' Rm_aa for the trace go there), w^2 [kmax], Cm [n][ldc] with
// ldc = n | 1: a lane's walk along its own row of Cm is free of bank conflicts for every n.  94 224 bytes at n = 63, kmax = 60.
// cnt[0] counts the cells without data (every output 0), cnt[1] those whose factorisation met a pivot that is not finite and
// > 0 (every output NaN).
template <typename KT>
__global__ __launch_bounds__(CL_WAVE) void k_column_res(int nx, int ny, int n, int kmax, int ldc, const KT *__restrict__ kern,
                                                        const float *__restrict__ wdat, double s2, double d2,
                                                        const float *__restrict__ depz, float *__restrict__ std_post,
                                                        float *__restrict__ std_noise, float *__restrict__ rdiag,
                                                        float *__restrict__ rsum, float *__restrict__ width,
                                                        float *__restrict__ rows, float *__restrict__ trace, int *__restrict__ cnt) {
  extern __shared__ double sm[];
  double *A = sm;
  double *K = A + n * n;
  double *w2 = K + kmax * n;
  double *Cm = w2 + kmax;
  const int t = threadIdx.x;
  const int nvx = nx - 2, ncell = nvx * (ny - 2);
  const int cell = blockIdx.x;
  const int j = cell / nvx, i = cell - j * nvx;
  const long ncol = (long)nx * ny, col = (long)(j + 1) * nx + (i + 1);
  const long o = (long)t * ncell + cell;

  auto fill = [&](float v) {                      // every output of this cell = v
    if (t < n) {
      std_post[o] = std_noise[o] = rdiag[o] = rsum[o] = v;
      if (width) width[o] = v;
    }
    if (rows)
      for (int q = t; q < n * n; q += CL_WAVE) rows[(long)q * ncell + cell] = v;
    if (trace && t == 0) trace[cell] = v;
  };
  bool data = false;
  if (t < kmax) {
    const float w = wdat ? wdat[(long)t * ncell + cell] : 1.0f;
    data = w != 0.0f;
    w2[t] = (double)w * (double)w;
  }
  if (!__any(data)) {
    fill(0.0f);
    if (t == 0) atomicAdd(cnt, 1);
    return;
  }
  for (int q = t; q < n * kmax; q += CL_WAVE) {   // q = l*kmax + p, the table's own order
    const int l = q / kmax, p = q - l * kmax;
    K[p * n + l] = (double)kern[(long)q * ncol + col];
  }
  __syncthreads();
  if (!dz_column_solve(t, n, kmax, 0, A, K, w2, nullptr, nullptr, s2, d2)) {
    fill(nanf(""));
    if (t == 0) atomicAdd(cnt + 1, 1);
    return;
  }
  double caa = 0.0;
  if (t < n) caa = dz_column_inverse_factor(t, n, A);
  __syncthreads();                                // (the other lanes divided by R_tt until here)
  if (t < n) A[t * n + t] = 1.0 / A[t * n + t];
  __syncthreads();
  double rd = 0.0;
  if (t < n) {
    const int a = t;
    double *Ca = Cm + a * ldc;
    for (int c = 0; c < n; c++) {
      double s = 0.0;
      for (int q = max(a, c); q < n; q++) s += A[a * n + q] * A[c * n + q];
      Ca[c] = c == a ? caa : s;
    }
    const double za = depz ? (double)depz[a] : 0.0;
    // (Rm C)_aa = (C K^T W^2 K C)_aa as the sum of squares sum_p w_p^2 (sum_c C_ac K_pc)^2: the difference C_aa - (C P C)_aa would lose
    // what is small against C_aa (a well determined direction under a weak regulariser)
    double nv = 0.0;
    for (int p = 0; p < kmax; p++)
      if (w2[p] != 0.0) {
        double u = 0.0;
        for (int c = 0; c < n; c++) u += Ca[c] * K[p * n + c];
        nv += w2[p] * (u * u);
      }
    double rs = 0.0, num = 0.0, den = 0.0;
    for (int c = 0; c < n; c++) {
      double s = 0.0;
      for (int e = max(c - 2, 0); e <= min(c + 2, n - 1); e++) s += Ca[e] * (s2 * dz_ltl(n, e, c) + (e == c ? d2 : 0.0));
      const double rm = (a == c ? 1.0 : 0.0) - s;
      if (rows) rows[((long)a * n + c) * ncell + cell] = (float)rm;
      rs += rm;
      if (depz) {
        const double dzc = (double)depz[c] - za;
        num += rm * rm * (dzc * dzc);
        den += rm * rm;
      }
      if (c == a) rd = rm;
    }
    std_post[o] = (float)sqrt(caa);
    std_noise[o] = (float)sqrt(nv);
    rdiag[o] = (float)rd;
    rsum[o] = (float)rs;
    if (width) width[o] = den > 0.0 ? (float)sqrt(num / den) : 0.0f;
  }
  if (trace) {
    __syncthreads();                              // (the lanes read K until here)
    if (t < n) K[t] = rd;
    __syncthreads();
    if (t == 0) {
      double s = 0.0;
      for (int a = 0; a < n; a++) s += K[a];
      trace[cell] = (float)s;
    }
  }
}

}  // namespace

int dz_column_stats(dazim_ctx *ctx, int ncell, int nrp, int kmax, const float *wdat, const double *part, float *out) {
  hipLaunchKernelGGL(k_column_stats, dim3((unsigned)nrp), dim3(CL_STATS_TB), 0, ctx->stream, ncell, kmax, wdat, part, out);
  DZ_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int dazim_vs_kernels(dazim_ctx *ctx, int nx, int ny, int nz, int kmax, const float *vel_u, const double *svs_u, const double *svp_u,
                     const double *srho_u, double *skern_u) {
  if (!ctx || nx < 1 || ny < 1 || nz < 1 || kmax < 1 || !vel_u || !svs_u || !svp_u || !srho_u || !skern_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_vs_kernels");
  DZ_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = dz_join_aux(ctx))) return rc;   // (the depth kernels may still be in the making: dazim_dispersion_kernels, disp.async)
  const size_t ncol = (size_t)nx * ny, nk = (size_t)nz * kmax * ncol;
  DzBuf<float> vel;
  DzBuf<double> svs, svp, srho, skern;
  if ((rc = vel.init(ctx, vel_u, (size_t)nz * ncol, true, false)) || (rc = svs.init(ctx, svs_u, nk, true, false)) ||
      (rc = svp.init(ctx, svp_u, nk, true, false)) || (rc = srho.init(ctx, srho_u, nk, true, false)) ||
      (rc = skern.init(ctx, skern_u, nk, false, true)))
    return rc;
  {
    DzTimer t(ctx, "vs_kernels");
    hipLaunchKernelGGL(k_vs_kernels, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, ctx->stream, (long)nk, kmax, (long)ncol,
                       vel.dev, svs.dev, svp.dev, srho.dev, skern.dev);
    DZ_HIP(hipGetLastError());
    t.stop();
  }
  if ((rc = skern.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int dazim_column_lsq(dazim_ctx *ctx, int nx, int ny, int nlay, int kmax, int kern_fp32, const void *kern_u, int nrhs,
                     const float *rhs_u, const float *wdat_u, float smooth, float damp, float *x_u, int *n_empty, float *stats) {
  if (!ctx || nx < 3 || ny < 3 || !kern_u || !rhs_u || !x_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_column_lsq");
  if (nlay < 1 || nlay > CL_MAXLAY) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_lsq: nlay %d outside 1..%d", nlay, CL_MAXLAY);
  if (kmax < 1 || kmax > CL_MAXPER) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_lsq: kmax %d outside 1..%d", kmax, CL_MAXPER);
  if (nrhs != 1 && nrhs != 2) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_lsq: nrhs %d is neither 1 nor 2", nrhs);
  if (!(smooth >= 0.0f) || !(damp >= 0.0f)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_lsq: negative smoothing or damping");
  if (smooth == 0.0f && damp == 0.0f) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_lsq: smoothing and damping both 0");
  DZ_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (nx - 2) * (ny - 2);
  const size_t nk = (size_t)nlay * kmax * nx * ny;
  DzBuf<double> kd;
  DzBuf<float> kf, rhs, wdat, x;
  if ((rc = kern_fp32 ? kf.init(ctx, (const float *)kern_u, nk, true, false) : kd.init(ctx, (const double *)kern_u, nk, true, false)) ||
      (rc = rhs.init(ctx, rhs_u, (size_t)nrhs * kmax * ncell, true, false)) ||
      (rc = wdat.init(ctx, wdat_u, wdat_u ? (size_t)kmax * ncell : 0, true, false)) ||
      (rc = x.init(ctx, x_u, (size_t)nrhs * nlay * ncell, false, true)))
    return rc;
  void *pe, *pp = nullptr, *ps = nullptr;
  if ((rc = dz_scratch(ctx, "col.empty", sizeof(int), &pe))) return rc;
  if (stats && ((rc = dz_scratch(ctx, "col.part", (size_t)nrhs * kmax * ncell * 2 * sizeof(double), &pp)) ||
                (rc = dz_scratch(ctx, "col.stats", (size_t)nrhs * kmax * 2 * sizeof(float), &ps))))
    return rc;
  DZ_HIP(hipMemsetAsync(pe, 0, sizeof(int), ctx->stream));
  const size_t lds = ((size_t)nlay * nlay + (size_t)kmax * nlay + kmax + (size_t)nrhs * kmax + (size_t)nrhs * nlay) * sizeof(double);
  const double s2 = (double)smooth * (double)smooth, d2 = (double)damp * (double)damp;
  {
    DzTimer t(ctx, "column_lsq");
    if (kern_fp32)
      hipLaunchKernelGGL(k_column_lsq<float>, dim3((unsigned)ncell), dim3(CL_WAVE), lds, ctx->stream, nx, ny, nlay, kmax, kf.dev, nrhs,
                         rhs.dev, wdat.dev, s2, d2, x.dev, (int *)pe, (double *)pp);
    else
      hipLaunchKernelGGL(k_column_lsq<double>, dim3((unsigned)ncell), dim3(CL_WAVE), lds, ctx->stream, nx, ny, nlay, kmax, kd.dev,
                         nrhs, rhs.dev, wdat.dev, s2, d2, x.dev, (int *)pe, (double *)pp);
    DZ_HIP(hipGetLastError());
    if (stats && (rc = dz_column_stats(ctx, ncell, nrhs * kmax, kmax, wdat.dev, (const double *)pp, (float *)ps))) return rc;
    t.stop();
  }
  int ne = 0;
  DZ_HIP(hipMemcpyAsync(&ne, pe, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (stats) DZ_HIP(hipMemcpyAsync(stats, ps, (size_t)nrhs * kmax * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = x.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_empty) *n_empty = ne;
  return 0;
}

int dazim_column_resolution(dazim_ctx *ctx, int nx, int ny, int nlay, int kmax, int kern_fp32, const void *kern_u, const float *wdat_u,
                            float smooth, float damp, const float *depz_u, float *std_post_u, float *std_noise_u, float *rdiag_u,
                            float *rsum_u, float *width_u, float *rows_u, float *trace_u, int *n_empty, int *n_failed) {
  if (!ctx || nx < 3 || ny < 3 || !kern_u || !std_post_u || !std_noise_u || !rdiag_u || !rsum_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_column_resolution");
  if (nlay < 1 || nlay > CL_MAXLAY) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_resolution: nlay %d outside 1..%d", nlay, CL_MAXLAY);
  if (kmax < 1 || kmax > CL_MAXPER) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_resolution: kmax %d outside 1..%d", kmax, CL_MAXPER);
  if (!(smooth >= 0.0f) || !(damp >= 0.0f)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_resolution: negative smoothing or damping");
  if (smooth == 0.0f && damp == 0.0f) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_resolution: smoothing and damping both 0");
  if (!width_u != !depz_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_resolution: width and depz go together (both or neither)");
  DZ_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (nx - 2) * (ny - 2), ldc = nlay | 1;
  const size_t nk = (size_t)nlay * kmax * nx * ny, no = (size_t)nlay * ncell;
  DzBuf<double> kd;
  DzBuf<float> kf, wdat, depz, sp, sn, rd, rs, wd, rw, tr;
  if ((rc = kern_fp32 ? kf.init(ctx, (const float *)kern_u, nk, true, false) : kd.init(ctx, (const double *)kern_u, nk, true, false)) ||
      (rc = wdat.init(ctx, wdat_u, wdat_u ? (size_t)kmax * ncell : 0, true, false)) ||
      (rc = depz.init(ctx, depz_u, depz_u ? (size_t)nlay : 0, true, false)) || (rc = sp.init(ctx, std_post_u, no, false, true)) ||
      (rc = sn.init(ctx, std_noise_u, no, false, true)) || (rc = rd.init(ctx, rdiag_u, no, false, true)) ||
      (rc = rs.init(ctx, rsum_u, no, false, true)) || (rc = wd.init(ctx, width_u, width_u ? no : 0, false, true)) ||
      (rc = rw.init(ctx, rows_u, rows_u ? no * nlay : 0, false, true)) || (rc = tr.init(ctx, trace_u, trace_u ? (size_t)ncell : 0, false, true)))
    return rc;
  void *pc;
  if ((rc = dz_scratch(ctx, "col.res_cnt", 2 * sizeof(int), &pc))) return rc;
  DZ_HIP(hipMemsetAsync(pc, 0, 2 * sizeof(int), ctx->stream));
  // A, K, w^2 and the rows of C: more than the 64 KiB a kernel gets unasked from n = 48 or so; a gfx950 workgroup may take 160 KiB
  const size_t lds = ((size_t)nlay * nlay + (size_t)kmax * nlay + kmax + (size_t)nlay * ldc) * sizeof(double);
  const void *kfn = kern_fp32 ? (const void *)k_column_res<float> : (const void *)k_column_res<double>;
  DZ_HIP(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (a refusal ends the call: no launch)
  const double s2 = (double)smooth * (double)smooth, d2 = (double)damp * (double)damp;
  {
    DzTimer t(ctx, "column_resolution");
    if (kern_fp32)
      hipLaunchKernelGGL(k_column_res<float>, dim3((unsigned)ncell), dim3(CL_WAVE), lds, ctx->stream, nx, ny, nlay, kmax, ldc, kf.dev,
                         wdat.dev, s2, d2, depz.dev, sp.dev, sn.dev, rd.dev, rs.dev, wd.dev, rw.dev, tr.dev, (int *)pc);
    else
      hipLaunchKernelGGL(k_column_res<double>, dim3((unsigned)ncell), dim3(CL_WAVE), lds, ctx->stream, nx, ny, nlay, kmax, ldc, kd.dev,
                         wdat.dev, s2, d2, depz.dev, sp.dev, sn.dev, rd.dev, rs.dev, wd.dev, rw.dev, tr.dev, (int *)pc);
    DZ_HIP(hipGetLastError());
    t.stop();
  }
  int cnt[2] = {0, 0};
  DZ_HIP(hipMemcpyAsync(cnt, pc, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = sp.finish()) || (rc = sn.finish()) || (rc = rd.finish()) || (rc = rs.finish()) || (rc = wd.finish()) || (rc = rw.finish()) ||
      (rc = tr.finish()))
    return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_empty) *n_empty = cnt[0];
  if (n_failed) *n_failed = cnt[1];
  return 0;
}

}  // extern "C"
