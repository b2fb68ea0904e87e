// surfdisp.hip -- the reference's surfdisp96 with EVERY value of its arguments, for a batch of layered models.
//
// The hot path (disp.hip) holds the one combination the reference's own programs use: spherical model, Rayleigh wave,
// fundamental mode, phase velocity (inv/CalSurfG.f90:1076-1077; Main_Jt.f90 STOPs on anything else).  The subroutine itself
// (inv/surfdisp96.f:52-354) also does Love waves (dltar1, :704-763), a water layer on top (dltar4's branch :844-860),
// higher modes (the loop :217-349) and group velocities (:226-233, :276-304) on a flat or a flattened spherical model;
// dazim_surfdisp96 offers all of it with the subroutine's own argument list, one lane per model.
//
// What runs where: the subroutine's prologue -- Earth flattening (sphere :480-547), the extremal velocities and the start
// value of the search (gtsolh :361-382), a few hundred host flops per model with the host libm's log / powf the reference
// calls -- is done on the host; the root searches (getsol :384-476, nevill :551-668 and the period equations) run on the
// device.  Both halves are surfdisp_device.h's functions, which disp_typed.hip and (the prologue's) disp.hip call as well; this
// file holds the subroutine's argument checks, the per-model arrays and the loops over modes and periods.  The device half is
// plain IEEE fp64, the reference's operations in the reference's order (this file is built with -ffp-contract=off like the
// rest of the library; no reciprocal / fused forms as in disp.hip's tuned dltar4).  What can
// differ from the reference is the last bit of the device's sin / cos / exp, i.e. roots that differ by ~1e-9 km/s before
// they are rounded to fp32: tests/test_surfdisp_full_gpu.py states the resulting bars.
#include <cmath>

#include "dazim_internal.h"
#include "surfdisp_device.h"

namespace {

using namespace dz_sd;   // surfdisp_device.h: everything of the subroutine that another unit runs as well

constexpr int NL = 200;  // inv/surfdisp96.f:57
constexpr int NP = 60;   // inv/surfdisp96.f:59

struct SdArgs {
  int nmodel, kmax, iwave, mode, igr;
  const float *d, *a, *b, *rho;   // [layer][model] flattened model (of this wave type)
  const int *mmax, *llw;          // [model]
  const float *betmx;             // [model]
  const double *cc;               // [model] start value of the search (= cm)
  const double *t;                // [kmax]
  double *c, *cb;                 // [k][model] scratch: roots of the current / previous mode at T (T/(1+h)) and at T/(1-h)
  double *cg;                     // [model][kmax] out
  int *nfail;                     // number of (model, period) entries left at 0
};

struct Model {
  const float *d, *a, *b, *rho;   // this lane's column of the [layer][model] arrays
  int stride, mmax, llw;
  __device__ float D(int m) const { return d[(size_t)(m - 1) * stride]; }
  __device__ float A(int m) const { return a[(size_t)(m - 1) * stride]; }
  __device__ float B(int m) const { return b[(size_t)(m - 1) * stride]; }
  __device__ float R(int m) const { return rho[(size_t)(m - 1) * stride]; }
};

// the loops over modes and periods, inv/surfdisp96.f:212-349, one lane per model
__global__ __launch_bounds__(64) void surfdisp_kernel(SdArgs S) {
  const int im = blockIdx.x * blockDim.x + threadIdx.x;
  if (im >= S.nmodel) return;
  Model M;
  M.d = S.d + im;
  M.a = S.a + im;
  M.b = S.b + im;
  M.rho = S.rho + im;
  M.stride = S.nmodel;
  M.mmax = S.mmax[im];
  M.llw = S.llw[im];
  const int ifunc = S.iwave, kmax = S.kmax, igr = S.igr;
  const float betmx = S.betmx[im];
  const double cc = S.cc[im];
  const double dc = fabs((double)ddc);
  const double cm = cc;
  double c1 = cc, clow = cc, del1st = 0.0;
  double *c = S.c + im, *cb = S.cb + im;
  double *cg = S.cg + (size_t)im * kmax;
  const size_t st = (size_t)S.nmodel;
  for (int i = 0; i < kmax; i++) {
    cb[i * st] = 0.0;
    c[i * st] = 0.0;
  }
  int ift = 999;
  for (int iq = 1; iq <= S.mode; iq++) {
    const int is = 1, ie = kmax;
    int k;
    bool failed = false;
    for (k = is; k <= ie; k++) {
      if (k >= ift) {
        failed = true;
        break;
      }
      int ifirst;   // the start values of mode iq at period k: from the previous period's root and the previous mode's (:247-266)
      if (k == is && iq == 1) {
        c1 = cc;
        clow = cc;
        ifirst = 1;
      } else if (k == is && iq > 1) {
        c1 = c[(is - 1) * st] + one * dc;
        clow = c1;
        ifirst = 1;
      } else if (k > is && iq > 1) {
        ifirst = 0;
        clow = c[(k - 1) * st] + one * dc;
        c1 = c[(k - 2) * st];
        if (c1 < clow) c1 = clow;
      } else {
        ifirst = 0;
        c1 = c[(k - 2) * st] - onea * dc;
        clow = cm;
      }
      double ck, ckb;
      float val;
      if (!period_step(M, S.t[k - 1], igr, ifunc, ifirst, c1, clow, igr > 0 ? cb[(k - 1) * st] + one * dc : 0.0, dc, cm, betmx, del1st,
                       ck, ckb, val)) {
        failed = true;
        break;
      }
      c[(k - 1) * st] = ck;
      if (igr > 0) cb[(k - 1) * st] = ckb;
      cg[k - 1] = (double)val;
    }
    if (failed) {  // :1700-1770
      ift = k;
      for (int i = k; i <= ie; i++) cg[i - 1] = 0.0;
    }
  }
  int nz = 0;
  for (int i = 0; i < kmax; i++)
    if (cg[i] == 0.0) nz++;
  if (nz) atomicAdd(S.nfail, nz);
}

}  // namespace

extern "C" int dazim_surfdisp96(dazim_ctx *ctx, int nmodel, int nlayer_max, const int *nlayer, const float *thk,
                                const float *vp, const float *vs, const float *rho, int iflsph, int iwave, int mode,
                                int igr, int kmax, const double *periods, double *cg, int *n_failed) {
  if (!ctx) return DAZIM_E_BAD_ARG;
  if (nmodel < 0 || !nlayer || !thk || !vp || !vs || !rho || !periods || !cg)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_surfdisp96: null argument");
  if (nlayer_max < 1 || nlayer_max > NL) return dz_fail(ctx, DAZIM_E_BAD_ARG, "nlayer_max=%d outside 1..%d (NL)", nlayer_max, NL);
  if (kmax < 1 || kmax > NP) return dz_fail(ctx, DAZIM_E_BAD_ARG, "kmax=%d outside 1..%d (NP)", kmax, NP);
  if (iwave != 1 && iwave != 2) return dz_fail(ctx, DAZIM_E_BAD_ARG, "iwave=%d: 1 (Love) or 2 (Rayleigh)", iwave);
  if (iflsph != 0 && iflsph != 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "iflsph=%d: 0 (flat) or 1 (spherical)", iflsph);
  if (mode < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "mode=%d: 1 = fundamental, 2 = first higher, ...", mode);
  if (n_failed) *n_failed = 0;
  if (nmodel == 0) return 0;
  DZ_HIP(hipSetDevice(ctx->device));
  // ---- inputs on the host (device pointers are copied back: the prologue is host arithmetic) ----
  const size_t nl = (size_t)nmodel * nlayer_max;
  std::vector<float> h_thk(nl), h_vp(nl), h_vs(nl), h_rho(nl);
  std::vector<int> h_n(nmodel);
  auto fetch = [&](void *dst, const void *src, size_t bytes) -> int {
    if (dz_is_device_ptr(src)) {
      DZ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    } else {
      memcpy(dst, src, bytes);
    }
    return 0;
  };
  int rc;
  if ((rc = fetch(h_thk.data(), thk, nl * 4)) || (rc = fetch(h_vp.data(), vp, nl * 4)) || (rc = fetch(h_vs.data(), vs, nl * 4)) ||
      (rc = fetch(h_rho.data(), rho, nl * 4)) || (rc = fetch(h_n.data(), nlayer, (size_t)nmodel * 4)))
    return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  // ---- the subroutine's prologue per model, inv/surfdisp96.f:93-211 ----
  std::vector<float> f_d(nl, 0.0f), f_a(nl, 1.0f), f_b(nl, 1.0f), f_r(nl, 1.0f), f_betmx(nmodel);
  std::vector<int> f_llw(nmodel);
  std::vector<double> f_cc(nmodel);
  for (int im = 0; im < nmodel; im++) {
    const int mmax = h_n[im];
    if (mmax < 1 || mmax > nlayer_max) return dz_fail(ctx, DAZIM_E_BAD_ARG, "model %d: nlayer=%d outside 1..%d", im, mmax, nlayer_max);
    float d[NL], a[NL], b[NL], r[NL];
    for (int i = 0; i < mmax; i++) {
      const size_t s = (size_t)im * nlayer_max + i;
      b[i] = h_vs[s];
      a[i] = h_vp[s];
      d[i] = h_thk[s];
      r[i] = h_rho[s];
    }
    int llw = 1;
    if (b[0] <= 0.0f) llw = 2;
    if (iflsph == 1) {  // sphere(0,0) then sphere(ifunc,1), :480-547
      double tmp[NL];
      sphere_flatten(mmax, 6370.0, d, tmp);
      for (int i = 0; i < mmax; i++) {
        a[i] = (float)((double)a[i] * tmp[i]);
        b[i] = (float)((double)b[i] * tmp[i]);
        r[i] = r[i] * (iwave == 1 ? rho_factor_love(tmp[i]) : rho_factor_rayleigh(tmp[i]));
      }
    }
    float betmx, cc1;
    startup(mmax, [&](int m, float &fa, float &fb) { fa = a[m - 1], fb = b[m - 1]; }, betmx, cc1);
    f_cc[im] = (double)cc1;
    f_betmx[im] = betmx;
    f_llw[im] = llw;
    for (int i = 0; i < mmax; i++) {
      const size_t s = (size_t)i * nmodel + im;
      f_d[s] = d[i];
      f_a[s] = a[i];
      f_b[s] = b[i];
      f_r[s] = r[i];
    }
  }
  // ---- device ----
  SdArgs S;
  S.nmodel = nmodel;
  S.kmax = kmax;
  S.iwave = iwave;
  S.mode = mode;
  S.igr = igr;
  void *p;
  auto up = [&](const char *name, const void *src, size_t bytes, const void **out) -> int {
    int r_ = dz_scratch(ctx, name, bytes, &p);
    if (r_) return r_;
    DZ_HIP(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    *out = p;
    return 0;
  };
  if ((rc = up("sd.d", f_d.data(), nl * 4, (const void **)&S.d)) || (rc = up("sd.a", f_a.data(), nl * 4, (const void **)&S.a)) ||
      (rc = up("sd.b", f_b.data(), nl * 4, (const void **)&S.b)) || (rc = up("sd.rho", f_r.data(), nl * 4, (const void **)&S.rho)) ||
      (rc = up("sd.mmax", h_n.data(), (size_t)nmodel * 4, (const void **)&S.mmax)) ||
      (rc = up("sd.llw", f_llw.data(), (size_t)nmodel * 4, (const void **)&S.llw)) ||
      (rc = up("sd.betmx", f_betmx.data(), (size_t)nmodel * 4, (const void **)&S.betmx)) ||
      (rc = up("sd.cc", f_cc.data(), (size_t)nmodel * 8, (const void **)&S.cc)) ||
      (rc = up("sd.t", periods, (size_t)kmax * 8, (const void **)&S.t)))
    return rc;
  if ((rc = dz_scratch(ctx, "sd.c", (size_t)nmodel * kmax, &S.c))) return rc;
  if ((rc = dz_scratch(ctx, "sd.cb", (size_t)nmodel * kmax, &S.cb))) return rc;
  if ((rc = dz_scratch(ctx, "sd.nfail", 4, &S.nfail))) return rc;
  DZ_HIP(hipMemsetAsync(S.nfail, 0, 4, ctx->stream));
  DzBuf<double> out;
  if ((rc = out.init(ctx, cg, (size_t)nmodel * kmax, false, true))) return rc;
  S.cg = out.dev;
  {
    DzTimer t(ctx, "surfdisp96");
    hipLaunchKernelGGL(surfdisp_kernel, dim3((unsigned)((nmodel + 63) / 64)), dim3(64), 0, ctx->stream, S);
    DZ_HIP(hipGetLastError());
    t.stop();
  }
  int nfail = 0;
  DZ_HIP(hipMemcpyAsync(&nfail, S.nfail, 4, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = out.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));   // (also: the host vectors above were the sources of asynchronous copies)
  if (n_failed) *n_failed = nfail;
  return 0;
}
