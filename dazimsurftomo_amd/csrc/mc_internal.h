// mc_internal.h -- what column_mc.hip (the handle, the step and the Vs and noise results), column_mc_aniso.hip (the Gc/Gs pass) and
// column_mc_radial.hip (the radial handle's setter, record state and result) share: the sampler's constants, the device view of a handle, the handle itself, the random numbers and the host helpers.
#pragma once
#include "dazim_internal.h"

constexpr int MC_WAVE = 64, MC_MAXLAY = 63, MC_MAXPER = 60, MC_MAXCHAIN = 64;
constexpr int MC_MAXGRP = 4;    // noise groups (dazim_mc_set_noise_groups)
constexpr int MC_MAXSEG = 4;    // segments (dazim_mc_set_segments): Rc, Rg, Lc, Lg
// Reflections of a proposal into its box.  u >= 2^-33 bounds |z| by sqrt(66 ln 2) < 6.77, and s <= 0.5 (dazim_mc_create refuses a
// larger start, the adaptation keeps it there) bounds the step by 3.39 box widths; each pass takes one width off the excess, so 4
// passes always suffice.  The cap and the clamp behind it only make the loop's bound visible: they never act on a valid handle.
// With the covariance proposal (kind 1) the step is s (hi - lo) y_k, y = L z: u in [0, 1] bounds C_kk, the squared norm of row k of L,
// by 1/4 + 1e-8; each Box-Muller pair has norm r <= 6.77, so |z|_2 <= 6.77 sqrt(ceil(nlay / 2)); s <= 2 / sqrt(nlay).  Together
// |s y_k| <= 2 * 0.50000001 * 6.77 * sqrt(ceil(nlay / 2) / nlay) < 6.78 box widths (the ratio is 1 at nlay = 1, less above): at most 7
// passes, still below the cap.
constexpr int MC_MAXFOLD = 8;
constexpr float MC_SMIN = 1e-3f, MC_SMAX = 0.5f;
// kind 1: states per knot a window must hold before it is factored, and the ridge on the diagonal of the covariance
constexpr int MC_COV_MIN = 8;
constexpr double MC_COV_RIDGE = 1e-8;

// Philox4x32-10 (Salmon et al., SC'11): c = counter in, block out; key (k0, k1) = the seed's low and high words
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
  for (int r = 0; r < 10; r++) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
  }
}

__device__ __forceinline__ void mc_block(unsigned w[4], long long step, unsigned gid, unsigned blk, unsigned long long seed) {
  w[0] = (unsigned)step;
  w[1] = gid;
  w[2] = blk;
  w[3] = 0u;
  philox4x32_10(w, (unsigned)seed, (unsigned)(seed >> 32));
}

__device__ __forceinline__ double mc_uniform(unsigned w) { return ((double)w + 0.5) * 2.3283064365386962890625e-10; }   // (w + 0.5) 2^-32

struct McDev {
  int nx, ny, nz, nlay, kmax, nchain, nbin, ncell, ncs;
  long ncol;
  unsigned long long seed;
  const int *cell_of;          // [ncs] inner-cell index of each sampled cell
  const int *cs_of;            // [ncell] sampled index of each inner cell, -1 = no data
  const float *vel0;           // [nz][ny][nx]
  const float *vmin, *vmax;    // [nlay][ncell]
  const float *cobs, *wdat;    // [kmax][ncell]
  float *cur, *prop;           // [nz][ncol]
  double *chi2;                // [ncol]
  float *scale;                // [ncs]
  int *acc_win;                // [ncs]
  double *sums;                // [2][nlay][ncol]
  unsigned *hist;              // [ncs][nlay][nbin]
  long long *accepted;         // [ncol]
  float *best;                 // [nlay][ncs]
  double *best_chi2;           // [ncs]
  unsigned long long *counters;   // [0] proposals without a root, [1] accepted moves of recorded steps
  // kind 1 only (null otherwise); npair = nlay (nlay + 1) / 2, pair (a, c), c <= a, at a (a + 1) / 2 + c
  long long *cov_n;            // [ncs] states in the sums
  double *cov_s1, *cov_s2;     // [ncs][nlay], [ncs][npair]: sums of u and of u_a u_c, u the state in box units
  double *chol;                // [ncs][npair]: the lower factor of the last covariance that factored
  int *cov_set;                // [ncs]: 1 once chol holds a factor
  // tempering only (ntemp = 1 and null otherwise); while it is on, scale [ncs] follows rung 0 of tscale
  int ntemp, nswap;
  const double *beta;          // [ntemp]
  float *tscale;               // [ncs][ntemp]
  int *tacc_win;               // [ncs][ntemp]
  long long *swap_try, *swap_acc;   // [ncs][ntemp - 1]
  // noise scales only (ngrp = 0 and null otherwise): ngrp groups of periods (dazim_mc_set_noise: the one group of every period),
  // lambda_g^2 ~ InverseGamma(ga0[g], gb0[g]) a priori
  int ngrp;
  float ga0[MC_MAXGRP], gb0[MC_MAXGRP];
  const int *grp;              // [kmax]: the group of every period
  double *chi2g;               // [ngrp][ncol], ngrp >= 2 only: chi^2_g of every chain's state (+inf before the first step)
  double *nsum;                // [2][ngrp][ncol]: sums of sqrt(B_g) and of B_g over the recorded states, B_g = gb0[g] + chi^2_g / 2
  long long *ncnt;             // [ncol]: states in them
  const double *ngam;          // [ngrp][MC_MAXPER + 1]: exp(lgamma(a - 0.5) - lgamma(a)) at a = ga0[g] + nd / 2, made on the host
  // Gaussian smoothness prior only (null and 0 otherwise): precision ps2 L^T L + pd2 I about pref, truncated by the box
  double ps2, pd2;             // (double)smooth^2, (double)damp^2
  const float *pref;           // [nlay][ncell]: the prior's centre
  double *pq;                  // [ncol]: the prior energy Q of every chain's state
  // radial anisotropy only (dazim_mc_set_radial; 0 and null otherwise): the knots are [Vsv_0..Vsv_{n-1}, Vsh_0..Vsh_{n-1}, deepest]
  int nrad;                    // n = nlay / 2
  double pm2;                  // (double)couple^2: the prior's mu^2 |vh - vv|^2
  float *vsv;                  // [n + 1][ncol]: the Vsv knots of prop beside a copy of its deepest row (rows n..2n of prop are Vsh's)
  double *rsum;                // [5][n][ncol]: sums of xi, xi^2, vv vh, V, V^2 over the recorded states
  long long *rgt1;             // [n][ncol]: recorded states with xi > 1
  unsigned *rhist;             // [ncs][n][nbin]: counts of xi over [(vmin_h / vmax_v)^2, (vmax_h / vmin_v)^2]
};

// Gc/Gs (dazim_mc_set_aniso).  Cold column cs * ncold + g is chain g * ntemp of sampled cell cs.
struct McAniso {
  const float *amap;           // [2][kmax][ncell]
  const float *wa;             // [kmax][ncell]
  double s2, d2;
  double *asum;                // [5][nlay][ncolc]
  double *avar;                // [nlay][ncolc]
  long long *acnt;             // [ncolc]
  long long *askip;            // [ncolc]: samples of the column that were skipped
};

struct dazim_mc {
  dazim_ctx *ctx = nullptr;
  McDev d{};
  int nadapt = 1;
  int kind = 0;             // the proposal: 0 isotropic in box units, 1 shaped by the chains' covariance
  float step0 = 0.0f;       // the initial step scale
  float tmax = 1.0f;        // tempering: the top rung's temperature (the ladder itself is in d)
  std::vector<double> beta{1.0};
  int64_t nstep = 0;        // steps done; 0 = the start models are drawn, not evaluated
  int64_t nburn_dec = 0;    // burn-in steps with a decision (the adaptation clock)
  int64_t nrec = 0, nrec_dec = 0;
  int n_empty = 0;
  double *pv = nullptr;     // [kmax][ncol]: the curves dazim_mc_run computes
  int nthin = 0;            // Gc/Gs: 0 = off, else one pass per nthin recorded steps of dazim_mc_run
  McAniso an{};             // ... its maps and sums (sized for ntemp = 1, so that any ladder fits)
  int64_t naniso = 0;       // ... samples taken
  int nseg = 1;             // dazim_mc_set_segments: the segments of the kmax periods (the default: Rayleigh phase alone)
  int seg_iwave[MC_MAXSEG] = {2, 0, 0, 0}, seg_igr[MC_MAXSEG] = {0, 0, 0, 0}, seg_kmax[MC_MAXSEG] = {0, 0, 0, 0};
  bool typed = false;       // ... other than Rayleigh phase alone: dazim_mc_run calls dazim_dispersion_kernels_typed
  int prior = 0;            // Gaussian smoothness prior: 0 = off (d.ps2, d.pd2, d.pref hold it while it is on)
  float psmooth = 0.0f, pdamp = 0.0f;
  float couple = 0.0f;      // dazim_mc_set_radial's mu (d.nrad > 0 marks a radial handle)
  int rad_nr = 0, rad_kr = 0;   // ... its Rayleigh segments (the first rad_nr) and their periods (rows [0, rad_kr) of pv)
  std::vector<void *> blocks;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

// a host copy of a host or device array
template <class T>
int mc_to_host(dazim_ctx *ctx, const T *p, size_t n, std::vector<T> &out) {
  out.resize(n);
  if (n == 0) return 0;
  if (dz_is_device_ptr(p)) {
    DZ_HIP(hipMemcpyAsync(out.data(), p, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    DZ_HIP(hipStreamSynchronize(ctx->stream));
  } else {
    memcpy(out.data(), p, n * sizeof(T));
  }
  return 0;
}

template <class T>
int mc_alloc(dazim_mc *mc, size_t n, T **out) {
  dazim_ctx *ctx = mc->ctx;
  void *p = nullptr;
  DZ_HIP(dz_malloc_retry(ctx, &p, (n ? n : 1) * sizeof(T)));
  mc->blocks.push_back(p);
  *out = (T *)p;
  return 0;
}

inline int mc_release(dazim_mc *mc) {
  for (void *p : mc->blocks) (void)hipFree(p);
  if (mc->e0) (void)hipEventDestroy(mc->e0);
  if (mc->e1) (void)hipEventDestroy(mc->e1);
  delete mc;
  return 0;
}

inline int mc_check(dazim_ctx *ctx, dazim_mc *mc, const char *what) {
  if (!ctx || !mc) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: null context or handle", what);
  if (mc->ctx != ctx) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: the handle belongs to another context", what);
  return 0;
}

inline long mc_ncolc(const dazim_mc *mc) { return (long)mc->d.ncs * (mc->d.nchain / mc->d.ntemp); }

// a *_state array for the caller (host or device memory), where they asked for it; enqueued on the ctx stream
inline hipError_t mc_get(dazim_ctx *ctx, void *dst, const void *src, size_t bytes) {
  return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, ctx->stream) : hipSuccess;
}

// ---- the Gc/Gs pass (column_mc_aniso.hip) as dazim_mc_run of column_mc.hip reaches it ------------------------------------------
#pragma GCC visibility push(hidden)
// one pass: the rung-0 states -> their curves -> their Lsen_Gsc -> one sample, in blocks of whole cells
int mc_aniso_pass(dazim_ctx *ctx, dazim_mc *mc, const float *depz, float sublayers, const double *periods);
int64_t mc_aniso_skipped(dazim_ctx *ctx, dazim_mc *mc, int *rc);   // the samples skipped so far, over all cold columns
// ---- the prior's record as dazim_mc_set_prior and dazim_mc_set_radial (column_mc_radial.hip) both bring it up to date ------------
// mc->prior from smooth, damp and couple; while it is on: pref (vref, or where the handle has none yet vel0's knots) and the Q of
// every chain's state into pq
int mc_prior_refresh(dazim_ctx *ctx, dazim_mc *mc, const std::vector<float> *vref);
#pragma GCC visibility pop
