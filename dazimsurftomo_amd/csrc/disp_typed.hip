// disp_typed.hip -- depthkernel (inv/CalSurfG.f90:1-139) for every wave type of its arguments iwave / igr: the dispersion curves
// and finite-difference depth kernels of Rayleigh group, Love phase and Love group velocities next to the Rayleigh phase velocities
// that disp.hip holds, as ONE table over "virtual periods" (the segments' periods laid end to end), which is all that the eikonal
// solver, the ray tracer, the G rows and the column solves index.
//
// A segment = one depthkernel call with its (iwave, igr): mode 1, iflsph 1, Brocher Vp / rho, refineGrid2LayerMdl, +-0.5 % copies.
//   (2, 0)  goes through dazim_dispersion_kernels (the tuned kernel) and lands in its slice: the same bits as that call.
//   others  typed_kernel below.  Work item = (segment, column, variant), one lane each; a workgroup is one wavefront that holds
//           up to 64 consecutive variants of one or a few columns of ONE segment, so the layer loop of the secular function has the
//           same trip count on every lane.  The root search is the subroutine's own, in the subroutine's order, by the functions
//           dazim_surfdisp96 runs (surfdisp_device.h: dltar1, dltar4, getsol, nevill and period_step, one period of the period
//           loop; plain IEEE fp64, no fused or reciprocal forms); typed_curve is that loop for mode 1.  What differs from
//           dazim_surfdisp96 is where the layers come from: not per-model global arrays filled by a host prologue, but two LDS
//           tables built by the wavefront from the column's knots -- a base table per column and, per lane, the few layers its one
//           perturbed knot touches (the layout of disp.hip's TableLayers) -- with the thickness-only Earth-flattening factors of
//           both wave types from a host table, filled by the functions that prologue calls (surfdisp_device.h: sphere_flatten,
//           rho_factor_*; also brocher, startup and the knots' layer ranges).  The layers are the ones the host prologue would have formed, bit for bit
//           (tests/test_disp_typed_gpu.py compares the tables with dazim_surfdisp96 on host-built stacks: equal).  The plans with
//           fewer than 64 items per workgroup are run by tests/test_disp_typed_shapes_gpu.py; a curves-only call (one base table per
//           item) takes them from 14 knots on at sublayers = 3 (32 items; 16 from 26 knots, 8 from 47).
//   Love    does not read Vp except through the start value of the first search (gtsolh of the slowest layer), which moves a root
//           by less than the search tolerance: sen_vp of a Love segment is defined as 0, and its 2 nz Vp copies are not run.
// A period without a root ends the curve (zeros from there on, counted in n_failed); the depth kernels of such an entry are 0.
#include <algorithm>
#include <cmath>

#include "dazim_internal.h"
#include "surfdisp_device.h"

namespace {

using namespace dz_sd;

constexpr int NL = 200;      // inv/surfdisp96.f:57
constexpr int NP = 60;       // inv/surfdisp96.f:59
constexpr int NZMAX = 64;    // knots per column, as dazim_dispersion_kernels
constexpr int TW = 64;       // lanes of a workgroup = one wavefront
constexpr int MAXSEG = 4;    // Rc, Rg, Lc, Lg
constexpr size_t LDS_MAX = 64 * 1024;

struct TLayer {  // per refined layer, geometry only (32 bytes)
  double tmp;    // (ar+ar)/(r0+r1), sphere() :528
  float d;       // flattened thickness, :524
  float rfac_r;  // btp**(-2.275): Rayleigh density factor, :541
  float rfac_l;  // btp**(-5) as 1/(x2*x2*x): Love density factor, :539 in the form of surfdisp.hip's prologue
  float fm, den; // (2j-1), 2*nsublay of refineGrid2LayerMdl (inv/CalSurfG.f90:2352)
  int iv;        // interval (1-based knot index); 0 for the half-space
};
static_assert(sizeof(TLayer) == 32, "TLayer is copied into LDS as 8 words");

struct TypedArgs {
  int ncol, nz, mmax, tw, npatch, cpb, nseg;   // tw: items per workgroup (lanes beyond it idle); cpb: columns a workgroup may span
  const float *vel;      // [nz][ncol]
  const TLayer *lay;     // [mmax]
  const double *t;       // [K] all virtual periods
  const int *krange;     // [nz + 1][2]: first layer (1-based) and number of layers that knot pi touches; pi = 0: none
  float *cg;             // per segment [ncol][nvar][kmax] from cgoff
  int iwave[MAXSEG], igr[MAXSEG], kmax[MAXSEG], koff[MAXSEG], nvar[MAXSEG];
  int blk0[MAXSEG + 1];  // first workgroup of each segment
  long long cgoff[MAXSEG];
};

// flattened layer m: Vp a, Vs b, density rho as surfdisp96 holds them after refineGrid2LayerMdl + sphere(0,0) + sphere(ifunc,1), from
// the column's knots kn [3][nz] (vs, vp, rho) with knot pi's quantity pq replaced by pval (pi = 0: none)
__device__ __forceinline__ void layer_model(const float *kn, int nz, int pi, int pq, float pval, const TLayer &L, bool love, float &a,
                                            float &b, float &rho) {
  auto get = [&](int q, int i) { return (i == pi && q == pq) ? pval : kn[q * nz + i - 1]; };
  float rvp, rvs, rrho;
  if (L.iv > 0) {
    const int i = L.iv;
    const float p0 = get(1, i), p1 = get(1, i + 1);
    const float s0 = get(0, i), s1 = get(0, i + 1);
    const float r0 = get(2, i), r1 = get(2, i + 1);
    rvp = p0 + L.fm * (p1 - p0) / L.den;
    rvs = s0 + L.fm * (s1 - s0) / L.den;
    rrho = r0 + L.fm * (r1 - r0) / L.den;
  } else {
    rvp = get(1, nz);
    rvs = get(0, nz);
    rrho = get(2, nz);
  }
  a = (float)((double)rvp * L.tmp);
  b = (float)((double)rvs * L.tmp);
  rho = rrho * (love ? L.rfac_l : L.rfac_r);
}

// a lane's layer stack for surfdisp_device.h: the column's base table, float4 (a, b, rho, d) per layer, except on the layers
// m_lo .. m_lo + cnt - 1 that the lane's perturbed knot touches, where (a, b, rho) come from the lane's rows of the patch table
// [npatch][tw][3]; d is the column's in any case.  Offsets in words from lds.
struct ColModel {
  const float *lds;
  int boff;       // layer m of the lane's column: lds[boff + 4 m]
  int poff, pst;  // layer m of the lane's own rows: lds[poff + pst m], pst = 3 tw
  int m_lo;
  unsigned cnt;
  int mmax, llw;
  __device__ __forceinline__ int row(int m) const { return (unsigned)(m - m_lo) < cnt ? poff + pst * m : boff + 4 * m; }
  __device__ __forceinline__ float A(int m) const { return lds[row(m)]; }
  __device__ __forceinline__ float B(int m) const { return lds[row(m) + 1]; }
  __device__ __forceinline__ float R(int m) const { return lds[row(m) + 2]; }
  __device__ __forceinline__ float D(int m) const { return lds[boff + 4 * m + 3]; }
};

// the loop over the periods of surfdisp96 for mode 1 (inv/surfdisp96.f:212-349 as surfdisp.hip's surfdisp_kernel states it, with
// iq = 1 only: the previous mode's roots are 0, the previous period's root is carried in a register); cg [kmax] fp32 = sngl(c) or U
__device__ void typed_curve(const ColModel &M, int ifunc, int igr, int kmax, const double *t, float betmx, float cc1, float *cg) {
  const double cc = (double)cc1;
  const double dc = fabs((double)ddc);
  const double cm = cc;
  double del1st = 0.0, cprev = 0.0, cb;
  int k;
  for (k = 1; k <= kmax; k++) {
    const bool first = k == 1;
    if (!period_step(M, t[k - 1], igr, ifunc, first ? 1 : 0, first ? cc : cprev - onea * dc, first ? cc : cm, 0.0 + one * dc, dc, cm, betmx,
                     del1st, cprev, cb, cg[k - 1]))
      break;
  }
  for (int i = k; i <= kmax; i++) cg[i - 1] = 0.0f;  // :1700-1770: no root at period k ends the curve
}

__global__ __launch_bounds__(TW) void typed_kernel(TypedArgs A) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];   // TLayer [mmax] | float4 base [cpb][mmax] | patch [npatch][tw][3] | knots [cpb][3][nz]
  const int lane = threadIdx.x, nz = A.nz, mmax = A.mmax, tw = A.tw;
  int seg = 0;
  while (seg + 1 < A.nseg && (int)blockIdx.x >= A.blk0[seg + 1]) seg++;
  const bool love = A.iwave[seg] == 1;
  const int nvar = A.nvar[seg], kmax = A.kmax[seg];
  const TLayer *s_lay = (const TLayer *)s_mem;
  float *s_base = s_mem + 8 * mmax;
  float *s_patch = s_base + 4 * A.cpb * mmax;
  float *s_knot = s_patch + 3 * A.npatch * tw;
  for (int i = lane; i < 8 * mmax; i += TW) s_mem[i] = ((const float *)A.lay)[i];
  const long nwork = (long)A.ncol * nvar;
  const long w0 = (long)((int)blockIdx.x - A.blk0[seg]) * tw;
  const int col0 = (int)(w0 / nvar);
  for (int i = lane; i < A.cpb * nz; i += TW) {
    const int c = i / nz, k = i - c * nz, col = col0 + c;
    if (col < A.ncol) {
      const float vs = A.vel[(size_t)k * A.ncol + col];
      float vp, rho;
      brocher(vs, vp, rho);
      s_knot[(c * 3 + 0) * nz + k] = vs;
      s_knot[(c * 3 + 1) * nz + k] = vp;
      s_knot[(c * 3 + 2) * nz + k] = rho;
    }
  }
  __syncthreads();
  for (int i = lane; i < A.cpb * mmax; i += TW) {   // the columns' own stacks
    const int c = i / mmax, m = i - c * mmax;
    if (col0 + c >= A.ncol) continue;
    float a, b, r;
    layer_model(s_knot + c * 3 * nz, nz, 0, -1, 0.0f, s_lay[m], love, a, b, r);
    s_base[4 * i + 0] = a;
    s_base[4 * i + 1] = b;
    s_base[4 * i + 2] = r;
    s_base[4 * i + 3] = s_lay[m].d;
  }
  const long w = w0 + lane;
  const bool active = lane < tw && w < nwork;
  const int col = active ? (int)(w / nvar) : col0;
  const int var = active ? (int)(w - (long)col * nvar) : 0;
  const float *kn = s_knot + (col - col0) * 3 * nz;
  // depthkernel's perturbation order: knot i, then (vs, vp, rho), then (-, +) (:76-124); a Love segment has no Vp copies
  int pi = 0, pq = -1;
  float pval = 0.0f;
  if (var > 0) {
    const int per = love ? 4 : 6, v1 = var - 1;
    pi = v1 / per + 1;
    const int r = v1 - (pi - 1) * per;
    pq = love ? (r >> 1) * 2 : r >> 1;
    const float b0 = kn[pq * nz + pi - 1];
    const float dln = 0.01f;
    pval = (r & 1) ? b0 + 0.5f * dln * b0 : b0 - 0.5f * dln * b0;
  }
  ColModel M;
  M.lds = s_mem;
  M.boff = (int)(s_base - s_mem) + 4 * (col - col0) * mmax - 4;
  M.pst = 3 * tw;
  M.m_lo = 0;
  M.cnt = 0u;
  M.mmax = mmax;
  M.llw = 1;   // Brocher's Vs > 0 model has no water layer
  if (pi > 0) {   // the layers knot pi touches (host table): the sublayers of intervals pi - 1 and pi, for the last knot also the half-space
    M.m_lo = A.krange[2 * pi];
    M.cnt = (unsigned)min(A.krange[2 * pi + 1], A.npatch);
  }
  M.poff = (int)(s_patch - s_mem) + 3 * lane - M.pst * M.m_lo;
  for (unsigned j = 0; j < M.cnt; j++) {
    float a, b, r;
    layer_model(kn, nz, pi, pq, pval, s_lay[M.m_lo + (int)j - 1], love, a, b, r);
    float *p = s_patch + ((size_t)j * tw + lane) * 3;
    p[0] = a;
    p[1] = b;
    p[2] = r;
  }
  __syncthreads();
  if (!active) return;
  float betmx, cc1;
  startup(mmax, [&](int m, float &fa, float &fb) { fa = M.A(m), fb = M.B(m); }, betmx, cc1);
  typed_curve(M, A.iwave[seg], A.igr[seg], kmax, A.t + A.koff[seg], betmx, cc1, A.cg + A.cgoff[seg] + (size_t)w * kmax);
}

// pv and the central differences of depthkernel (inv/CalSurfG.f90:60,90-133) of one segment into its slice of the tables:
// ((double)cg2 - (double)cg1) / (double)(0.01f * base) as disp.hip forms them; 0 where the column's own curve has ended, and for
// the Vp kernel of a Love segment
__global__ void typed_finalize(int ncol, int nz, int kmax, int nvar, int love, int K, int koff, const float *__restrict__ vel,
                               const float *__restrict__ cg, double *__restrict__ pv, double *__restrict__ svs,
                               double *__restrict__ svp, double *__restrict__ srho, int *nfail) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (long)ncol * kmax) return;
  const int k = (int)(tid / ncol), col = (int)(tid - (long)k * ncol);
  const float *c = cg + (size_t)col * nvar * kmax;
  const float c0 = c[k];
  pv[(size_t)(koff + k) * ncol + col] = (double)c0;
  if (c0 == 0.0f) atomicAdd(nfail, 1);
  if (!svs) return;
  const float dln = 0.01f;
  const int per = love ? 4 : 6;
  for (int i = 0; i < nz; i++) {
    const float vs = vel[(size_t)i * ncol + col];
    float vp, rho;
    brocher(vs, vp, rho);
    const float base[3] = {vs, vp, rho};
    double *out[3] = {svs, svp, srho};
    for (int q = 0; q < 3; q++) {
      double s = 0.0;
      if (c0 != 0.0f && !(love && q == 1)) {
        const int v = 1 + i * per + (love ? q : q * 2);   // (Love: vs at 0, rho at 2)
        const float cg1 = c[(size_t)v * kmax + k], cg2 = c[(size_t)(v + 1) * kmax + k];
        s = ((double)cg2 - (double)cg1) / (double)(dln * base[q]);
      }
      out[q][((size_t)i * K + koff + k) * ncol + col] = s;
    }
  }
}

const char *type_name(int iwave, int igr) { return iwave == 2 ? (igr ? "Rayleigh group" : "Rayleigh phase") : (igr ? "Love group" : "Love phase"); }

}  // namespace

extern "C" int dazim_dispersion_kernels_typed(dazim_ctx *ctx, int nx, int ny, int nz, const float *vel_u, const float *depz,
                                              float sublayers, int nseg, const int *seg_iwave, const int *seg_igr,
                                              const int *seg_kmax, const double *periods, double *pv_u, double *svs_u,
                                              double *svp_u, double *srho_u, int *n_failed) {
  if (!ctx) return DAZIM_E_BAD_ARG;
  if (!vel_u || !depz || !seg_iwave || !seg_igr || !seg_kmax || !periods || !pv_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_dispersion_kernels_typed: null argument");
  if (nz < 2 || nz > NZMAX || nx < 1 || ny < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad nx/ny/nz");
  if (nseg < 1 || nseg > MAXSEG) return dz_fail(ctx, DAZIM_E_BAD_ARG, "nseg=%d outside 1..%d", nseg, MAXSEG);
  const int ngiven = (svs_u ? 1 : 0) + (svp_u ? 1 : 0) + (srho_u ? 1 : 0);
  if (ngiven != 0 && ngiven != 3) return dz_fail(ctx, DAZIM_E_BAD_ARG, "sen_vs, sen_vp, sen_rho: all three or none");
  int K = 0, irc = -1;   // virtual periods; the Rayleigh-phase segment, if any
  int koff[MAXSEG];
  for (int s = 0; s < nseg; s++) {
    if (seg_iwave[s] != 1 && seg_iwave[s] != 2) return dz_fail(ctx, DAZIM_E_BAD_ARG, "segment %d: iwave=%d: 1 (Love) or 2 (Rayleigh)", s, seg_iwave[s]);
    if (seg_igr[s] != 0 && seg_igr[s] != 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "segment %d: igr=%d: 0 (phase) or 1 (group)", s, seg_igr[s]);
    if (seg_kmax[s] < 1 || seg_kmax[s] > NP) return dz_fail(ctx, DAZIM_E_BAD_ARG, "segment %d: kmax=%d outside 1..%d (NP)", s, seg_kmax[s], NP);
    for (int q = 0; q < s; q++)
      if (seg_iwave[q] == seg_iwave[s] && seg_igr[q] == seg_igr[s])
        return dz_fail(ctx, DAZIM_E_BAD_ARG, "segments %d and %d are both %s", q, s, type_name(seg_iwave[s], seg_igr[s]));
    if (seg_iwave[s] == 2 && seg_igr[s] == 0) irc = s;
    koff[s] = K;
    K += seg_kmax[s];
  }
  // Rayleigh phase alone: the tuned call as it is
  if (nseg == 1 && irc == 0)
    return dazim_dispersion_kernels(ctx, nx, ny, nz, vel_u, depz, sublayers, seg_kmax[0], periods, pv_u, svs_u, svp_u, srho_u, n_failed);
  if (n_failed) *n_failed = 0;
  DZ_HIP(hipSetDevice(ctx->device));
  const bool kernels = ngiven == 3;
  const int ncol = nx * ny;
  const size_t nk = (size_t)nz * K * ncol;
  int rc;
  if ((rc = dz_fmm_finish(ctx)) || (rc = dz_join_aux(ctx))) return rc;
  DzBuf<float> vel;
  DzBuf<double> pv, svs, svp, srho;
  if ((rc = vel.init(ctx, vel_u, (size_t)nz * ncol, true, false)) || (rc = pv.init(ctx, pv_u, (size_t)K * ncol, false, true))) return rc;
  if (kernels && ((rc = svs.init(ctx, svs_u, nk, false, true)) || (rc = svp.init(ctx, svp_u, nk, false, true)) || (rc = srho.init(ctx, srho_u, nk, false, true))))
    return rc;
  int nfail_rc = 0;
  if (irc >= 0) {   // the Rayleigh-phase slice: the tuned call on device arrays, its depth kernels through a compact table into their rows
    const int kr = seg_kmax[irc];
    const size_t nkr = (size_t)nz * kr * ncol;
    double *tmp = nullptr;
    if (kernels && (rc = dz_scratch(ctx, "dispt.rc", 3 * nkr, &tmp))) return rc;
    if ((rc = dazim_dispersion_kernels(ctx, nx, ny, nz, vel.dev, depz, sublayers, kr, periods + koff[irc], pv.dev + (size_t)koff[irc] * ncol,
                                       kernels ? tmp : nullptr, kernels ? tmp + nkr : nullptr, kernels ? tmp + 2 * nkr : nullptr, &nfail_rc)))
      return rc;
    if (kernels) {
      if ((rc = dz_join_aux(ctx))) return rc;   // (option disp.async: the perturbed copies may still be running)
      double *dst[3] = {svs.dev, svp.dev, srho.dev};
      for (int q = 0; q < 3; q++)
        DZ_HIP(hipMemcpy2DAsync(dst[q] + (size_t)koff[irc] * ncol, (size_t)K * ncol * 8, tmp + q * nkr, (size_t)kr * ncol * 8, (size_t)kr * ncol * 8,
                                (size_t)nz, hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  // ---- the other segments: geometry-only layer table, refineGrid2LayerMdl (inv/CalSurfG.f90:2339-2365) + sphere (:510-545) ----
  std::vector<TLayer> lay;
  std::vector<float> thk;
  for (const DzRefinedLayer &R : dz_refine_layers(depz, nz, sublayers)) {
    TLayer L{};
    L.iv = R.iv, L.fm = R.fm, L.den = R.den;
    lay.push_back(L);
    thk.push_back(R.thk);
  }
  const int mmax = (int)lay.size();
  if (mmax > NL) return dz_fail(ctx, DAZIM_E_BAD_ARG, "refined model has %d layers > NL=%d", mmax, NL);
  std::vector<double> tmp(mmax);
  sphere_flatten(mmax, 6370.0, thk.data(), tmp.data());
  for (int i = 0; i < mmax; i++)
    lay[i].d = thk[i], lay[i].tmp = tmp[i], lay[i].rfac_r = rho_factor_rayleigh(tmp[i]), lay[i].rfac_l = rho_factor_love(tmp[i]);
  TypedArgs A{};
  A.ncol = ncol, A.nz = nz, A.mmax = mmax;
  std::vector<int> krange(2 * (NZMAX + 1), 0);
  const int longest = knot_layer_ranges(lay, nz, krange.data());
  A.npatch = kernels ? longest : 0;   // (a curves-only call has no perturbed knots: no patch table)
  int nvar_min = 1 << 30;
  size_t ncg = 0;
  for (int s = 0; s < nseg; s++) {
    if (s == irc) continue;
    const int g = A.nseg++;
    A.iwave[g] = seg_iwave[s], A.igr[g] = seg_igr[s], A.kmax[g] = seg_kmax[s], A.koff[g] = koff[s];
    A.nvar[g] = kernels ? 1 + (seg_iwave[s] == 1 ? 4 : 6) * nz : 1;
    A.cgoff[g] = (long long)ncg;
    ncg += (size_t)ncol * A.nvar[g] * A.kmax[g];
    nvar_min = std::min(nvar_min, A.nvar[g]);
  }
  // items per workgroup: a wavefront's 64, fewer where the tables of that many items do not fit the LDS (very many layers or knots)
  size_t lds = 0;
  for (A.tw = TW; A.tw >= 1; A.tw /= 2) {
    A.cpb = (A.tw + nvar_min - 1) / nvar_min + 1;
    lds = ((size_t)8 * mmax + (size_t)4 * A.cpb * mmax + (size_t)3 * A.npatch * A.tw + (size_t)3 * A.cpb * nz) * sizeof(float);
    if (lds <= LDS_MAX) break;
  }
  if (A.tw < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_dispersion_kernels_typed: %d layers x %d knots do not fit the LDS", mmax, nz);
  A.blk0[0] = 0;
  for (int g = 0; g < A.nseg; g++) A.blk0[g + 1] = A.blk0[g] + (int)(((long)ncol * A.nvar[g] + A.tw - 1) / A.tw);
  for (int g = A.nseg; g < MAXSEG; g++) A.blk0[g + 1] = A.blk0[A.nseg];
  A.vel = vel.dev;
  double *d_t = nullptr;
  TLayer *d_lay = nullptr;
  int *d_nfail = nullptr, *d_krange = nullptr;
  if ((rc = dz_scratch(ctx, "dispt.krange", (size_t)2 * (NZMAX + 1), &d_krange)) || (rc = dz_scratch(ctx, "dispt.lay", (size_t)NL, &d_lay)) || (rc = dz_scratch(ctx, "dispt.t", (size_t)MAXSEG * NP, &d_t)) ||
      (rc = dz_scratch(ctx, "dispt.cg", ncg, &A.cg)) || (rc = dz_scratch(ctx, "dispt.nfail", 4, &d_nfail)))
    return rc;
  DZ_HIP(hipMemcpyAsync(d_lay, lay.data(), sizeof(TLayer) * mmax, hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync(d_t, periods, sizeof(double) * K, hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync(d_krange, krange.data(), sizeof(int) * krange.size(), hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemsetAsync(d_nfail, 0, 4, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));   // (lay and krange are locals: their copies are over before they go)
  A.lay = d_lay, A.t = d_t, A.krange = d_krange;
  {
    DzTimer t(ctx, "disp_typed");
    hipLaunchKernelGGL(typed_kernel, dim3((unsigned)A.blk0[A.nseg]), dim3(TW), lds, ctx->stream, A);
    DZ_HIP(hipGetLastError());
    for (int g = 0; g < A.nseg; g++) {
      hipLaunchKernelGGL(typed_finalize, dim3((unsigned)(((long)ncol * A.kmax[g] + 255) / 256)), dim3(256), 0, ctx->stream, ncol, nz, A.kmax[g],
                         A.nvar[g], A.iwave[g] == 1 ? 1 : 0, K, A.koff[g], vel.dev, A.cg + A.cgoff[g], pv.dev, kernels ? svs.dev : nullptr,
                         kernels ? svp.dev : nullptr, kernels ? srho.dev : nullptr, d_nfail);
      DZ_HIP(hipGetLastError());
    }
    t.stop();
  }
  ctx->ksec["disp_typed.items_per_wg"] = A.tw;
  int nfail = 0;
  DZ_HIP(hipMemcpyAsync(&nfail, d_nfail, 4, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = pv.finish()) || (rc = svs.finish()) || (rc = svp.finish()) || (rc = srho.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_failed) *n_failed = nfail + nfail_rc;
  return 0;
}
