// column_mc_radial.hip -- radial anisotropy in the Monte-Carlo sampler (dazim_mc_set_radial): the handle's
// knots are the stacked vector [Vsv_0..Vsv_{n-1}, Vsh_0..Vsh_{n-1}, deepest], which k_mc_step<.., RAD = 1> of column_mc.hip samples as
// it samples any knots.  Here: the setter (the Vsv model beside the proposals, the record's arrays, the prior's Q brought up to date
// through mc_prior_refresh), the copies of the record, and k_mc_radial_final, which turns the record into the posterior of xi =
// (Vsh / Vsv)^2, of the Voigt average and the Vsv-Vsh correlation per inner cell and knot.  dazim_mc_run's two dispersion calls per
// step are column_mc.hip's.
#include "mc_internal.h"

#include <cmath>

namespace {

// posterior statistics of the derived quantities, one wavefront per inner cell, lane = knot pair a < n.  Every fp64 sum runs over
// the recorded (rung-0) chains in chain order inside the lane, as in k_mc_final; the counts are integers.  Every output is nullable.
__global__ __launch_bounds__(MC_WAVE) void k_mc_radial_final(McDev M, long long nrec, float *__restrict__ xi_mean,
                                                             float *__restrict__ xi_std, float *__restrict__ xi_q,
                                                             float *__restrict__ xi_rhat, float *__restrict__ p_gt1,
                                                             float *__restrict__ corr_vh, float *__restrict__ voigt_mean,
                                                             float *__restrict__ voigt_std) {
  const int cell = blockIdx.x, a = threadIdx.x, n = M.nrad;
  if (a >= n) return;
  const int cs = M.cs_of[cell], nvx = M.nx - 2, j = cell / nvx, i = cell - j * nvx;
  const long c0 = (long)(j + 1) * M.nx + (i + 1), nxy = (long)M.nx * M.ny, o = (long)a * M.ncell + cell, nk = (long)n * M.ncell;
  if (cs < 0) {   // no data: the start model's xi and Voigt average
    const double vv = (double)M.vel0[(long)a * nxy + c0], vh = (double)M.vel0[(long)(n + a) * nxy + c0];
    const double r = vh / vv, xi = r * r, V = sqrt((2.0 * vv * vv + vh * vh) / 3.0);
    if (xi_mean) xi_mean[o] = (float)xi;
    if (xi_std) xi_std[o] = 0.0f;
    if (xi_q)
      for (int e = 0; e < 3; e++) xi_q[e * nk + o] = (float)xi;
    if (xi_rhat) xi_rhat[o] = NAN;
    if (p_gt1) p_gt1[o] = NAN;
    if (corr_vh) corr_vh[o] = NAN;
    if (voigt_mean) voigt_mean[o] = (float)V;
    if (voigt_std) voigt_std[o] = 0.0f;
    return;
  }
  const double N = (double)nrec, Mc = (double)(M.nchain / M.ntemp), tot = N * Mc;
  const long nn = (long)n * M.ncol;
  double s1 = 0.0, s2 = 0.0, sm = 0.0, sv = 0.0, svv = 0.0, sh = 0.0, shh = 0.0, svh = 0.0, g1 = 0.0, g2 = 0.0;
  long long gt = 0;
  for (int ch = 0; ch < M.nchain; ch += M.ntemp) {
    const long col = (long)cs * M.nchain + ch, oc = (long)a * M.ncol + col;
    const double x1 = M.rsum[oc];
    s1 += x1;
    s2 += M.rsum[nn + oc];
    sm += x1 / N;
    svh += M.rsum[2 * nn + oc];
    g1 += M.rsum[3 * nn + oc];
    g2 += M.rsum[4 * nn + oc];
    gt += M.rgt1[oc];
    sv += M.sums[(long)a * M.ncol + col];
    svv += M.sums[((long)M.nlay + a) * M.ncol + col];
    sh += M.sums[(long)(n + a) * M.ncol + col];
    shh += M.sums[((long)M.nlay + n + a) * M.ncol + col];
  }
  const double mu = s1 / tot;
  if (xi_mean) xi_mean[o] = (float)mu;
  if (xi_std) xi_std[o] = (float)sqrt(fmax(s2 / tot - mu * mu, 0.0));
  if (xi_rhat) {   // R-hat as k_mc_final forms it, on the chains' sums of xi
    double W = 0.0, B = 0.0;
    const double mbar = sm / Mc;
    for (int ch = 0; ch < M.nchain; ch += M.ntemp) {
      const long oc = (long)a * M.ncol + (long)cs * M.nchain + ch;
      const double x1 = M.rsum[oc], x2 = M.rsum[nn + oc];
      const double mj = x1 / N;
      W += (x2 - N * mj * mj) / (N - 1.0);
      B += (mj - mbar) * (mj - mbar);
    }
    W /= Mc;
    B *= N / (Mc - 1.0);
    xi_rhat[o] = (M.nchain / M.ntemp > 1 && nrec > 1 && W > 0.0) ? (float)sqrt(((N - 1.0) / N * W + B / N) / W) : NAN;
  }
  if (xi_q) {   // 2.5 / 50 / 97.5 % from the counts, linear inside a bin, over the knot pair's exact range of xi
    const unsigned *h = M.rhist + ((long)cs * n + a) * M.nbin;
    const double rl = (double)M.vmin[(long)(n + a) * M.ncell + cell] / (double)M.vmax[o];
    const double rh = (double)M.vmax[(long)(n + a) * M.ncell + cell] / (double)M.vmin[o];
    const double lo = rl * rl, hi = rh * rh;
    const double qs[3] = {0.025, 0.5, 0.975};
    for (int e = 0; e < 3; e++) {
      const double target = qs[e] * tot;
      double cum = 0.0, pos = (double)M.nbin;
      for (int b = 0; b < M.nbin; b++) {
        const double nb = (double)h[b];
        if (nb > 0.0 && cum + nb >= target) {
          pos = (double)b + (target - cum) / nb;
          break;
        }
        cum += nb;
      }
      xi_q[e * nk + o] = (float)(lo + pos * (hi - lo) / (double)M.nbin);
    }
  }
  if (p_gt1) p_gt1[o] = (float)((double)gt / tot);
  if (corr_vh) {
    const double ev = sv / tot, eh = sh / tot;
    const double dv = sqrt(fmax(svv / tot - ev * ev, 0.0)), dh = sqrt(fmax(shh / tot - eh * eh, 0.0));
    corr_vh[o] = (dv > 0.0 && dh > 0.0) ? (float)((svh / tot - ev * eh) / (dv * dh)) : NAN;
  }
  const double gm = g1 / tot;
  if (voigt_mean) voigt_mean[o] = (float)gm;
  if (voigt_std) voigt_std[o] = (float)sqrt(fmax(g2 / tot - gm * gm, 0.0));
}

}  // namespace

extern "C" {

int dazim_mc_set_radial(dazim_ctx *ctx, dazim_mc *mc, float couple) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_set_radial"))) return rc;
  if (!(std::isfinite(couple) && couple >= 0.0f))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_radial: couple %g is not finite and >= 0", couple);
  if (mc->nstep > 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_radial: the handle has done %lld steps", (long long)mc->nstep);
  McDev &M = mc->d;
  if (M.nlay % 2 != 0)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_radial: %d sampled knots are not n Vsv knots and n Vsh knots", M.nlay);
  if (mc->nthin > 0)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_radial: the handle samples Gc/Gs (dazim_mc_set_aniso), which takes one Vs profile");
  int nr = 0, kr = 0;
  while (nr < mc->nseg && mc->seg_iwave[nr] == 2) kr += mc->seg_kmax[nr++];
  bool ok = nr > 0 && nr < mc->nseg;
  for (int s = nr; s < mc->nseg; s++) ok = ok && mc->seg_iwave[s] == 1;
  if (!ok)
    return dz_fail(ctx, DAZIM_E_BAD_ARG,
                   "dazim_mc_set_radial: dazim_mc_set_segments has not given at least one Rayleigh and one Love segment with every "
                   "Rayleigh segment before every Love segment");
  DZ_HIP(hipSetDevice(ctx->device));
  std::vector<float> vmin;
  if ((rc = mc_to_host(ctx, M.vmin, (size_t)M.nlay * M.ncell, vmin))) return rc;
  for (size_t e = 0; e < vmin.size(); e++)
    if (!(vmin[e] > 0.0f))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_radial: vmin %g <= 0 at knot %d, cell %d: xi has no range", vmin[e],
                     (int)(e / M.ncell), (int)(e % M.ncell));
  const int n = M.nlay / 2;
  const size_t nc = (size_t)M.ncol, nh = (size_t)M.ncs * n * M.nbin;
  if (!M.vsv) {
    if ((rc = mc_alloc(mc, (size_t)(n + 1) * nc, &M.vsv)) || (rc = mc_alloc(mc, (size_t)5 * n * nc, &M.rsum)) ||
        (rc = mc_alloc(mc, (size_t)n * nc, &M.rgt1)) || (rc = mc_alloc(mc, nh, &M.rhist)))
      return rc;
  }
  if (nc > 0) {   // the start models are the proposals until the first step: their Vsv knots and the deepest row
    DZ_HIP(hipMemcpyAsync(M.vsv, M.prop, (size_t)n * nc * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    DZ_HIP(hipMemcpyAsync(M.vsv + (size_t)n * nc, M.prop + (size_t)M.nlay * nc, nc * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    DZ_HIP(hipMemsetAsync(M.rsum, 0, (size_t)5 * n * nc * sizeof(double), ctx->stream));
    DZ_HIP(hipMemsetAsync(M.rgt1, 0, (size_t)n * nc * sizeof(long long), ctx->stream));
    DZ_HIP(hipMemsetAsync(M.rhist, 0, nh * sizeof(unsigned), ctx->stream));
  }
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  M.nrad = n;
  M.pm2 = (double)couple * (double)couple;
  mc->couple = couple;
  mc->rad_nr = nr;
  mc->rad_kr = kr;
  return mc_prior_refresh(ctx, mc, nullptr);
}

int dazim_mc_radial_models(dazim_mc *mc, float **vsv_dev, float **vsh_dev, int64_t *ncol) {
  if (!mc || mc->d.nrad == 0) return DAZIM_E_BAD_ARG;
  if (vsv_dev) *vsv_dev = mc->d.vsv;
  if (vsh_dev) *vsh_dev = mc->d.prop + (size_t)mc->d.nrad * mc->d.ncol;
  if (ncol) *ncol = mc->d.ncol;
  return 0;
}

int dazim_mc_radial_state(dazim_ctx *ctx, dazim_mc *mc, int *n, float *couple, double *rsum, int64_t *ngt1, unsigned *xhist) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_radial_state"))) return rc;
  const McDev &M = mc->d;
  if (n) *n = M.nrad;
  if (couple) *couple = mc->couple;
  if (!M.nrad) {
    if (rsum || ngt1 || xhist) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_radial_state: the handle is not radial (dazim_mc_set_radial)");
    return 0;
  }
  DZ_HIP(hipSetDevice(ctx->device));
  DZ_HIP(mc_get(ctx, rsum, M.rsum, (size_t)5 * M.nrad * M.ncol * 8));
  DZ_HIP(mc_get(ctx, ngt1, M.rgt1, (size_t)M.nrad * M.ncol * 8));
  DZ_HIP(mc_get(ctx, xhist, M.rhist, (size_t)M.ncs * M.nrad * M.nbin * 4));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int dazim_mc_radial_result(dazim_ctx *ctx, dazim_mc *mc, float *xi_mean_u, float *xi_std_u, float *xi_q_u, float *xi_rhat_u,
                           float *p_gt1_u, float *corr_vh_u, float *voigt_mean_u, float *voigt_std_u) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_radial_result"))) return rc;
  const McDev &M = mc->d;
  if (!M.nrad) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_radial_result: the handle is not radial (dazim_mc_set_radial)");
  if (M.ncs > 0 && mc->nrec < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_radial_result: no recorded step yet");
  DZ_HIP(hipSetDevice(ctx->device));
  const size_t nk = (size_t)M.nrad * M.ncell;
  DzBuf<float> xm, xs, xq, xr, pg, cr, vm, vs;
  if ((rc = xm.init(ctx, xi_mean_u, nk, false, true)) || (rc = xs.init(ctx, xi_std_u, nk, false, true)) ||
      (rc = xq.init(ctx, xi_q_u, 3 * nk, false, true)) || (rc = xr.init(ctx, xi_rhat_u, nk, false, true)) ||
      (rc = pg.init(ctx, p_gt1_u, nk, false, true)) || (rc = cr.init(ctx, corr_vh_u, nk, false, true)) ||
      (rc = vm.init(ctx, voigt_mean_u, nk, false, true)) || (rc = vs.init(ctx, voigt_std_u, nk, false, true)))
    return rc;
  hipLaunchKernelGGL(k_mc_radial_final, dim3((unsigned)M.ncell), dim3(MC_WAVE), 0, ctx->stream, M, (long long)mc->nrec, xm.dev, xs.dev,
                     xq.dev, xr.dev, pg.dev, cr.dev, vm.dev, vs.dev);
  DZ_HIP(hipGetLastError());
  if ((rc = xm.finish()) || (rc = xs.finish()) || (rc = xq.finish()) || (rc = xr.finish()) || (rc = pg.finish()) || (rc = cr.finish()) ||
      (rc = vm.finish()) || (rc = vs.finish()))
    return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
