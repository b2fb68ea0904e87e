// column.hip -- the second step of the two-step method: from per-period maps to a depth model, cell by cell.
//
// dazim_vs_kernels: the dc/dVs table the 3-D rows multiply (k_row_kernels of rays.hip, through the same dz_row_kernel).
// dazim_column_lsq: one small regularised dense least-squares problem per inner map cell, all cells in one launch: one wavefront
// per cell builds its normal matrix (at most 63 x 63) in LDS, factors it by Cholesky and solves, all in fp64.  The launch is bound
// by latency (a few MB of kernel table in all), so it stays this plain.  Every sum runs in a fixed order: the same inputs give the
// same bits, whether they come from the host or the device.
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

}  // namespace

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
    if (stats) {
      hipLaunchKernelGGL(k_column_stats, dim3((unsigned)(nrhs * kmax)), dim3(CL_STATS_TB), 0, ctx->stream, ncell, kmax, wdat.dev,
                         (const double *)pp, (float *)ps);
      DZ_HIP(hipGetLastError());
    }
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

}  // extern "C"
