// column_mc_aniso.hip -- Gc/Gs posteriors from the Monte-Carlo Vs chains of column_mc.hip (dazim_mc_set_aniso).
//
// Conditional on a Vs column the Gc/Gs posterior is the Gaussian of dazim_column_lsq's normal equations, so the chains' thinned
// rung-0 states give its marginal by averaging the conditional mean and covariance (Rao-Blackwellisation).  k_mc_gather copies the
// rung-0 states into a compact table, k_mc_aniso solves one wavefront per such column with dz_column_solve and adds to the column's
// own sums, k_mc_aniso_final reduces them per cell.  The pass only reads the chains.
#include "mc_internal.h"

#include <algorithm>
#include <cmath>

namespace {

// cold columns c0 .. c0 + nb - 1 of the current states into out [nz][nb]
__global__ void k_mc_gather(McDev M, long c0, long nb, float *__restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M.nz * nb) return;
  const long k = i / nb, cc = c0 + (i - k * nb);
  const int ncold = M.nchain / M.ntemp;
  const long cs = cc / ncold, g = cc - cs * ncold;
  out[i] = M.cur[k * M.ncol + cs * M.nchain + g * M.ntemp];
}

// One sample of the Gc/Gs sums, one wavefront per cold column c0 + blockIdx.x; lsen [nlay][kmax][nb] holds that column at index
// blockIdx.x.  LDS as k_column_lsq with nrhs = 2.  After dz_column_solve lane k forms column k of R^-1 by itself, in the unused
// strict upper triangle of A (row k), and with it (A^-1)_kk: dz_column_inverse_factor, which k_column_res of column.hip calls too.
__global__ __launch_bounds__(MC_WAVE) void k_mc_aniso(McDev M, McAniso S, const float *__restrict__ lsen, long c0, long nb) {
  extern __shared__ double mc_lds[];
  const int n = M.nlay, kmax = M.kmax, t = threadIdx.x;
  double *A = mc_lds;
  double *K = A + n * n;
  double *w2 = K + kmax * n;
  double *wr = w2 + kmax;
  double *b = wr + 2 * kmax;
  const int ncold = M.nchain / M.ntemp;
  const long lc = blockIdx.x, cc = c0 + lc, ncolc = (long)M.ncs * ncold;
  const long cs = cc / ncold, g = cc - cs * ncold;
  const int cell = M.cell_of[cs];
  if (isinf(M.chi2[cs * M.nchain + g * M.ntemp])) {   // the chain has no curve yet: no sample
    if (t == 0) S.askip[cc] += 1;
    return;
  }
  if (t < kmax) {
    const float w = S.wa[(long)t * M.ncell + cell];
    const double ww = (double)w * (double)w;
    w2[t] = ww;
    for (int r = 0; r < 2; r++) wr[r * kmax + t] = w != 0.0f ? ww * (double)S.amap[((long)r * kmax + t) * M.ncell + cell] : 0.0;
  }
  for (int q = t; q < n * kmax; q += MC_WAVE) {   // q = l*kmax + p, the table's own order
    const int l = q / kmax, p = q - l * kmax;
    K[p * n + l] = (double)lsen[(long)q * nb + lc];
  }
  __syncthreads();
  const bool ok = dz_column_solve(t, n, kmax, 2, A, K, w2, wr, b, S.s2, S.d2);
  if (!ok) {
    if (t == 0) S.askip[cc] += 1;
    return;
  }
  if (t < n) {
    const int k = t;
    const double dg = dz_column_inverse_factor(k, n, A);
    const double xc = b[k], xs = b[n + k];
    const long o = (long)k * ncolc + cc, pl = (long)n * ncolc;
    S.asum[o] += xc;
    S.asum[pl + o] += xs;
    S.asum[2 * pl + o] += xc * xc;
    S.asum[3 * pl + o] += xs * xs;
    S.asum[4 * pl + o] += xc * xs;
    S.avar[o] += dg;
  }
  if (t == 0) S.acnt[cc] += 1;
}

// the Gc/Gs statistics, one wavefront per inner cell, lane = knot; the cold columns of the cell in column order inside the lane
__global__ __launch_bounds__(MC_WAVE) void k_mc_aniso_final(McDev M, McAniso S, float *__restrict__ mean, float *__restrict__ stdv,
                                                            float *__restrict__ stdb, float *__restrict__ cov,
                                                            long long *__restrict__ nsamp) {
  const int cell = blockIdx.x, k = threadIdx.x;
  const int cs = M.cs_of[cell];
  const long o = (long)k * M.ncell + cell, nk = (long)M.nlay * M.ncell;
  if (cs < 0) {
    if (k < M.nlay) {
      mean[o] = mean[nk + o] = 0.0f;
      stdv[o] = stdv[nk + o] = 0.0f;
      stdb[o] = stdb[nk + o] = 0.0f;
      cov[o] = 0.0f;
    }
    if (k == 0) nsamp[cell] = 0;
    return;
  }
  const int ncold = M.nchain / M.ntemp;
  const long ncolc = (long)M.ncs * ncold, pl = (long)M.nlay * ncolc;
  long long cnt = 0;
  for (int g = 0; g < ncold; g++) cnt += S.acnt[(long)cs * ncold + g];
  if (k == 0) nsamp[cell] = cnt;
  if (k >= M.nlay) return;
  if (cnt == 0) {
    mean[o] = mean[nk + o] = 0.0f;
    stdv[o] = stdv[nk + o] = NAN;
    stdb[o] = stdb[nk + o] = NAN;
    cov[o] = NAN;
    return;
  }
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, sv = 0.0;
  for (int g = 0; g < ncold; g++) {
    const long c = (long)k * ncolc + (long)cs * ncold + g;
    for (int e = 0; e < 5; e++) s[e] += S.asum[e * pl + c];
    sv += S.avar[c];
  }
  const double dn = (double)cnt, within = sv / dn;
  const double mc = s[0] / dn, ms = s[1] / dn;
  const double bc = fmax(s[2] / dn - mc * mc, 0.0), bs = fmax(s[3] / dn - ms * ms, 0.0);
  mean[o] = (float)mc;
  mean[nk + o] = (float)ms;
  stdv[o] = (float)sqrt(within + bc);
  stdv[nk + o] = (float)sqrt(within + bs);
  stdb[o] = (float)sqrt(bc);
  stdb[nk + o] = (float)sqrt(bs);
  cov[o] = (float)(s[4] / dn - mc * ms);
}

// one Gc/Gs sample of the cold columns c0 .. c0 + nb - 1 from lsen [nlay][kmax][nb] (device); enqueued, no host wait
int mc_launch_aniso(dazim_ctx *ctx, dazim_mc *mc, const float *lsen, long c0, long nb) {
  const McDev &M = mc->d;
  if (nb <= 0) return 0;
  const size_t lds = ((size_t)M.nlay * M.nlay + (size_t)M.kmax * M.nlay + 3 * (size_t)M.kmax + 2 * (size_t)M.nlay) * sizeof(double);
  hipLaunchKernelGGL(k_mc_aniso, dim3((unsigned)nb), dim3(MC_WAVE), lds, ctx->stream, M, mc->an, lsen, c0, nb);
  DZ_HIP(hipGetLastError());
  return 0;
}

// the bytes dazim_ti_kernels keeps per column in its two large scratch arrays (ti.up, ti.prt of ti.hip)
size_t mc_ti_bytes_per_column(const dazim_mc *mc, const float *depz, float sublayers) {
  return dz_refine_layers(depz, mc->d.nz, sublayers).size() * 10 * sizeof(double) * (size_t)mc->d.kmax;
}

}  // namespace

int mc_aniso_pass(dazim_ctx *ctx, dazim_mc *mc, const float *depz, float sublayers, const double *periods) {
  const McDev &M = mc->d;
  const int ncold = M.nchain / M.ntemp;
  // cells per block: option mc.aniso_block_cells, else what keeps the TI scratch below 2 GiB
  long bc = dz_opt(ctx, "mc.aniso_block_cells", 0);
  if (bc <= 0) bc = (long)(((size_t)2 << 30) / (mc_ti_bytes_per_column(mc, depz, sublayers) * (size_t)ncold));
  bc = std::min(std::max(bc, 1L), (long)M.ncs);
  const size_t nbmax = (size_t)bc * ncold;
  float *cold, *lsen;
  double *pvc;
  int rc;
  if ((rc = dz_scratch(ctx, "mc.aniso.cold", (size_t)M.nz * nbmax, &cold)) ||
      (rc = dz_scratch(ctx, "mc.aniso.pv", (size_t)M.kmax * nbmax, &pvc)) ||
      (rc = dz_scratch(ctx, "mc.aniso.lsen", (size_t)M.nlay * M.kmax * nbmax, &lsen)))
    return rc;
  for (long cs0 = 0; cs0 < M.ncs; cs0 += bc) {
    const long nb = std::min(bc, (long)M.ncs - cs0) * ncold, c0 = cs0 * ncold;
    const long ng = (long)M.nz * nb;
    hipLaunchKernelGGL(k_mc_gather, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, ctx->stream, M, c0, nb, cold);
    DZ_HIP(hipGetLastError());
    int nf = 0;
    if ((rc = dazim_dispersion_kernels(ctx, (int)nb, 1, M.nz, cold, depz, sublayers, M.kmax, periods, pvc, nullptr, nullptr, nullptr,
                                       &nf)) ||
        (rc = dazim_ti_kernels(ctx, (int)nb, 1, M.nz, cold, depz, sublayers, M.kmax, periods, pvc, lsen)) ||
        (rc = mc_launch_aniso(ctx, mc, lsen, c0, nb)))
      return rc;
    DZ_HIP(hipStreamSynchronize(ctx->stream));   // the next block overwrites the scratch tables
  }
  mc->naniso++;
  return 0;
}

int64_t mc_aniso_skipped(dazim_ctx *ctx, dazim_mc *mc, int *rc) {
  std::vector<long long> sk((size_t)mc_ncolc(mc));
  *rc = 0;
  if (sk.empty()) return 0;
  const hipError_t e = hipMemcpy(sk.data(), mc->an.askip, sk.size() * sizeof(long long), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    *rc = dz_fail(ctx, -(int)e - 1000, "dazim_mc aniso: %s", hipGetErrorString(e));
    return 0;
  }
  int64_t n = 0;
  for (long long v : sk) n += v;
  return n;
}

extern "C" {

int dazim_mc_set_aniso(dazim_ctx *ctx, dazim_mc *mc, int nthin, const float *amap_u, const float *wa_u, float smooth, float damp) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_set_aniso"))) return rc;
  if (nthin < 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_aniso: nthin %d < 0", nthin);
  if (mc->nstep > 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_aniso: the handle has done %lld steps", (long long)mc->nstep);
  if (nthin == 0) {
    mc->nthin = 0;
    return 0;
  }
  if (mc->d.nrad > 0)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_aniso: the handle is radial (dazim_mc_set_radial): Gc/Gs takes one Vs profile");
  if (mc->typed)
    return dz_fail(ctx, DAZIM_E_BAD_ARG,
                   "dazim_mc_set_aniso: the Gc/Gs kernel Lsen_Gsc is Rayleigh-phase, and the handle's segments (dazim_mc_set_segments) "
                   "are not Rayleigh phase alone");
  if (!amap_u || !wa_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_set_aniso");
  if (!(smooth >= 0.0f) || !(damp >= 0.0f)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_aniso: negative smoothing or damping");
  if (smooth == 0.0f && damp == 0.0f) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_aniso: smoothing and damping both 0");
  DZ_HIP(hipSetDevice(ctx->device));
  McDev &M = mc->d;
  const size_t nw = (size_t)M.kmax * M.ncell;
  std::vector<float> amap, wa;
  if ((rc = mc_to_host(ctx, amap_u, 2 * nw, amap)) || (rc = mc_to_host(ctx, wa_u, nw, wa))) return rc;
  for (size_t e = 0; e < amap.size(); e++)
    if (!std::isfinite(amap[e]))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_aniso: a non-finite amap at period %d, cell %d", (int)(e / M.ncell % M.kmax),
                     (int)(e % M.ncell));
  for (size_t e = 0; e < wa.size(); e++)
    if (!std::isfinite(wa[e]))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_aniso: a non-finite wa at period %d, cell %d", (int)(e / M.ncell),
                     (int)(e % M.ncell));
  McAniso &S = mc->an;
  const size_t nc = (size_t)M.ncol, nl = (size_t)M.nlay;
  if (!S.asum) {
    float *am, *w;
    if ((rc = mc_alloc(mc, 2 * nw, &am)) || (rc = mc_alloc(mc, nw, &w)) || (rc = mc_alloc(mc, 5 * nl * nc, &S.asum)) ||
        (rc = mc_alloc(mc, nl * nc, &S.avar)) || (rc = mc_alloc(mc, nc, &S.acnt)) || (rc = mc_alloc(mc, nc, &S.askip)))
      return rc;
    S.amap = am;
    S.wa = w;
  }
  DZ_HIP(hipMemcpyAsync((void *)S.amap, amap.data(), 2 * nw * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync((void *)S.wa, wa.data(), nw * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemsetAsync(S.asum, 0, (5 * nl * nc ? 5 * nl * nc : 1) * sizeof(double), ctx->stream));
  DZ_HIP(hipMemsetAsync(S.avar, 0, (nl * nc ? nl * nc : 1) * sizeof(double), ctx->stream));
  DZ_HIP(hipMemsetAsync(S.acnt, 0, (nc ? nc : 1) * sizeof(long long), ctx->stream));
  DZ_HIP(hipMemsetAsync(S.askip, 0, (nc ? nc : 1) * sizeof(long long), ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  S.s2 = (double)smooth * (double)smooth;
  S.d2 = (double)damp * (double)damp;
  mc->nthin = nthin;
  mc->naniso = 0;
  return 0;
}

int dazim_mc_aniso_step(dazim_ctx *ctx, dazim_mc *mc, int kmax, int64_t ncolc, const float *lsen_u) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_aniso_step"))) return rc;
  if (mc->nthin < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_aniso_step: dazim_mc_set_aniso has not switched Gc/Gs on");
  if (mc->nstep < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_aniso_step: the handle has not done a step yet");
  if (kmax != mc->d.kmax || ncolc != mc_ncolc(mc))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_aniso_step: kernels [%d][%lld] for a handle of [%d][%ld]", kmax, (long long)ncolc,
                   mc->d.kmax, mc_ncolc(mc));
  if (!lsen_u && ncolc > 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_aniso_step");
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_join_aux(ctx))) return rc;
  DzBuf<float> lsen;
  if ((rc = lsen.init(ctx, lsen_u, (size_t)mc->d.nlay * kmax * ncolc, true, false))) return rc;
  {
    DzTimer t(ctx, "mc_aniso");
    if ((rc = mc_launch_aniso(ctx, mc, lsen.dev, 0, (long)ncolc))) return rc;
    t.stop();
  }
  mc->naniso++;
  return 0;
}

int dazim_mc_aniso_state(dazim_ctx *ctx, dazim_mc *mc, int *nthin, double *asum, double *avar, int64_t *acnt, int64_t *skipped) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_aniso_state"))) return rc;
  if (nthin) *nthin = mc->nthin;
  if (mc->nthin < 1) {
    if (asum || avar || acnt || skipped)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_aniso_state: dazim_mc_set_aniso has not switched Gc/Gs on");
    return 0;
  }
  DZ_HIP(hipSetDevice(ctx->device));
  const McAniso &S = mc->an;
  const size_t nc = (size_t)mc_ncolc(mc), nl = (size_t)mc->d.nlay;
  DZ_HIP(mc_get(ctx, asum, S.asum, 5 * nl * nc * 8));
  DZ_HIP(mc_get(ctx, avar, S.avar, nl * nc * 8));
  DZ_HIP(mc_get(ctx, acnt, S.acnt, nc * 8));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (skipped) {
    *skipped = mc_aniso_skipped(ctx, mc, &rc);
    if (rc) return rc;
  }
  return 0;
}

int dazim_mc_aniso_result(dazim_ctx *ctx, dazim_mc *mc, float *mean_u, float *std_u, float *stdb_u, float *cov_u, int64_t *nsamp_u) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_aniso_result"))) return rc;
  if (!mean_u || !std_u || !stdb_u || !cov_u || !nsamp_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_aniso_result");
  if (mc->nthin < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_aniso_result: dazim_mc_set_aniso has not switched Gc/Gs on");
  if (mc->naniso < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_aniso_result: no Gc/Gs sample yet");
  DZ_HIP(hipSetDevice(ctx->device));
  const McDev &M = mc->d;
  const size_t nk = (size_t)M.nlay * M.ncell;
  DzBuf<float> mean, stdv, stdb, cov;
  DzBuf<long long> ns;
  if ((rc = mean.init(ctx, mean_u, 2 * nk, false, true)) || (rc = stdv.init(ctx, std_u, 2 * nk, false, true)) ||
      (rc = stdb.init(ctx, stdb_u, 2 * nk, false, true)) || (rc = cov.init(ctx, cov_u, nk, false, true)) ||
      (rc = ns.init(ctx, (const long long *)nsamp_u, (size_t)M.ncell, false, true)))
    return rc;
  hipLaunchKernelGGL(k_mc_aniso_final, dim3((unsigned)M.ncell), dim3(MC_WAVE), 0, ctx->stream, M, mc->an, mean.dev, stdv.dev, stdb.dev,
                     cov.dev, ns.dev);
  DZ_HIP(hipGetLastError());
  if ((rc = mean.finish()) || (rc = stdv.finish()) || (rc = stdb.finish()) || (rc = cov.finish()) || (rc = ns.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
