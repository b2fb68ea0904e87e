// column_mc.hip -- Monte-Carlo Vs per map cell: random-walk Metropolis chains on the knots of each cell's
// Vs column, every chain resident on the device, the forward model the unchanged dispersion kernel (dazim_dispersion_kernels,
// curves only, one column per chain).
//
// k_mc_init draws the start models from the prior; k_mc_step runs one wavefront per sampled cell, one lane per chain: chi^2 of the
// curves of the proposals, accept / reject, record, adapt the step scale, draw the next proposals; k_mc_final turns the records into
// the posterior statistics.  Random numbers are Philox4x32-10 keyed on the seed and counted by (step, chain, block): the results
// depend on the seed and the inputs only.  Sums across chains run over the lanes in chain order inside one lane (k_mc_final); the
// histogram counts are the only atomics, on integers.
//
// Parallel tempering (dazim_mc_set_tempering): chain ch is rung ch % ntemp of replica group ch / ntemp, rung r samples the posterior
// to the power beta_r, and neighbouring rungs of a group exchange their states.  A group's rungs are neighbouring lanes of the cell's
// wavefront, so a swap is a lane shuffle inside k_mc_step<KIND, 1>; only the rung-0 chains are recorded.
//
// Gc/Gs posteriors (dazim_mc_set_aniso) are column_mc_aniso.hip's: a pass that only reads the chains, and that dazim_mc_run reaches
// through mc_internal.h, which also holds the handle, its device view McDev, the constants and the random numbers.
//
// Noise scales integrated out (dazim_mc_set_noise_groups, G <= 4 groups of periods; dazim_mc_set_noise is the one group of every
// period): the data std of a period of group g is lambda_g / w_p with lambda_g^2 ~ InverseGamma(a0_g, b0_g), and every lambda_g is
// integrated out in closed form.  k_mc_step<KIND, TEMPER, NG> takes every decision on the energy X = sum_g 2 a_g log(B_g), B_g = b0_g +
// chi^2_g / 2, a_g = a0_g + nd_g / 2, over the groups with data in the cell, in place of chi^2 (mc_energy); mc_chi2 forms chi^2_g
// beside chi^2 in the one loop over the periods, chi2g [G][ncol] keeps the chi^2_g of every chain's state (G >= 2; one group's is
// chi2), each recorded rung-0 lane adds sqrt(B_g) and B_g of its state to its own columns, and k_mc_noise_final turns those sums into
// the posterior mean and std of lambda_g per (group, cell) (Rao-Blackwellisation again).
//
// Typed data (dazim_mc_set_segments): dazim_mc_run computes the proposals' curves with dazim_dispersion_kernels_typed, the handle's
// periods being the virtual periods of the segments laid end to end; the step never asks what kind of wave a period is.
//
// Gaussian smoothness prior (dazim_mc_set_prior): dazim_column_lsq's regulariser read as a prior, exp(-Q / 2) with Q = d^T (smooth^2
// L^T L + damp^2 I) d, d the state's knots minus a reference, inside the box.  k_mc_step<KIND, TEMPER, NG, 1> takes every decision
// on E + Q in place of E (mc_total, mc_prior_q; a rung samples (likelihood x Gaussian prior)^beta) and keeps the Q of every chain's state
// in pq [ncol].  The best model stays the one of lowest raw chi^2: the best-fitting model, not the maximum a posteriori.
//
// Radial anisotropy (dazim_mc_set_radial, column_mc_radial.hip): the knots are the stacked [Vsv, Vsh, deepest], which the step samples
// as any knots.  k_mc_step<KIND, TEMPER, NG, PRIOR, 1> takes Q from mc_prior_q_radial, records xi = (Vsh / Vsv)^2, the Voigt average and
// Vsv Vsh of every recorded state, and stores a proposed Vsv knot to the Vsv model as well, which dazim_mc_run computes the Rayleigh
// segments' curves from (the Love segments' come from rows n..2n of the proposals): two dazim_dispersion_kernels_typed calls per step.
#include "mc_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>

namespace {

// NG: the compile-time bound of the noise groups, 0 (the fixed noise level), 1 or MC_MAXGRP; group g < NG is on
template <int NG>
__device__ __forceinline__ bool mc_group_on(const McDev &M, int g) { return NG == 1 || g < M.ngrp; }

// the total chi^2 of column col's curves, the sum in period order, and for NG >= 1 beside it chi^2_g of every group (each in period
// order within its group: the other groups add nothing) and nd_g, the group's periods with data in the cell.  A period with data and
// no root makes the total and its group +inf (NG 0 stops there: nothing else is counted)
template <int NG>
__device__ __forceinline__ double mc_chi2(const McDev &M, const double *__restrict__ pv, int cell, long col, double (&cg)[NG ? NG : 1],
                                          int (&ndg)[NG ? NG : 1]) {
  double chi2 = 0.0;
  for (int p = 0; p < M.kmax; p++) {
    const float w = M.wdat[(long)p * M.ncell + cell];
    if (w == 0.0f) continue;
    const int gp = NG > 1 ? M.grp[p] : 0;
#pragma unroll
    for (int g = 0; g < NG; g++) ndg[g] += gp == g;
    const double c = pv[(long)p * M.ncol + col];
    if (c == 0.0) {
      chi2 = INFINITY;
      if constexpr (NG == 0) break;
#pragma unroll
      for (int g = 0; g < NG; g++)
        if (gp == g) cg[g] = INFINITY;
      continue;
    }
    const double r = (double)w * ((double)M.cobs[(long)p * M.ncell + cell] - c);
    const double rr = r * r;
    chi2 += rr;
#pragma unroll
    for (int g = 0; g < NG; g++)
      if (gp == g) cg[g] += rr;
  }
  return chi2;
}

// the energy a decision is taken on: chi^2 itself, or with the noise scales integrated out X = sum over the groups with ndg[g] > 0, in
// group order from 0.0, of 2 a_g log(B_g(chi^2_g)), a_g = a0_g + ndg[g] / 2; +inf where the total chi^2 is (a chi^2_g is +inf only then)
template <int NG>
__device__ __forceinline__ double mc_energy(const McDev &M, const int (&ndg)[NG ? NG : 1], const double (&cg)[NG ? NG : 1], double chi2) {
  if constexpr (NG == 0) {
    return chi2;
  } else {
    if (isinf(chi2)) return INFINITY;
    double x = 0.0;
#pragma unroll
    for (int g = 0; g < NG; g++)
      if (mc_group_on<NG>(M, g) && ndg[g] > 0) x += 2.0 * ((double)M.ga0[g] + 0.5 * ndg[g]) * log((double)M.gb0[g] + 0.5 * cg[g]);
    return x;
  }
}

// what a decision compares: the energy, with the prior plus Q
template <int PRIOR>
__device__ __forceinline__ double mc_total(double x, double q) {
  if constexpr (PRIOR) return x + q;
  else return x;
}

// the prior energy Q = ps2 |L d|^2 + pd2 |d|^2 of column col of v [nz][ncol] (cur or prop), d = v - pref over the nlay sampled knots;
// row a of L is 2 d_a at both ends and (2 d_a - d_{a-1}) - d_{a+1} between them (dz_ltl's L).  fp64, both sums in knot order
__device__ __forceinline__ double mc_prior_q(const McDev &M, const float *__restrict__ v, long col, int cell) {
  const int n = M.nlay;
  double q1 = 0.0, q2 = 0.0, dm = 0.0;
  double d = (double)v[col] - (double)M.pref[cell];
  for (int a = 0; a < n; a++) {
    const double dp = a + 1 < n ? (double)v[(a + 1) * M.ncol + col] - (double)M.pref[(long)(a + 1) * M.ncell + cell] : 0.0;
    const double t = (a == 0 || a == n - 1) ? 2.0 * d : (2.0 * d - dm) - dp;
    q1 += t * t;
    q2 += d * d;
    dm = d;
    d = dp;
  }
  return M.ps2 * q1 + M.pd2 * q2;
}

// the same of a radial handle's stacked knots (dazim_mc_set_radial): q1 and q2 run on through both profiles in knot order, L's rule
// inside each profile of n knots (knots n - 1 and n are ends: no row crosses the boundary), and qc = |vh - vv|^2 over the n pairs in
// knot order; Q = (ps2 q1 + pd2 q2) + pm2 qc
__device__ __forceinline__ double mc_prior_q_radial(const McDev &M, const float *__restrict__ v, long col, int cell) {
  const int n = M.nrad;
  double q1 = 0.0, q2 = 0.0, qc = 0.0;
  for (int h = 0; h < 2; h++) {
    const int k0 = h * n;
    double dm = 0.0;
    double d = (double)v[k0 * M.ncol + col] - (double)M.pref[(long)k0 * M.ncell + cell];
    for (int a = 0; a < n; a++) {
      const double dp =
          a + 1 < n ? (double)v[(k0 + a + 1) * M.ncol + col] - (double)M.pref[(long)(k0 + a + 1) * M.ncell + cell] : 0.0;
      const double t = (a == 0 || a == n - 1) ? 2.0 * d : (2.0 * d - dm) - dp;
      q1 += t * t;
      q2 += d * d;
      dm = d;
      d = dp;
    }
  }
  for (int a = 0; a < n; a++) {
    const double c = (double)v[(n + a) * M.ncol + col] - (double)v[a * M.ncol + col];
    qc += c * c;
  }
  return (M.ps2 * q1 + M.pd2 * q2) + M.pm2 * qc;
}

// the lanes of rung r: chains r, r + ntemp, ..
__device__ __forceinline__ unsigned long long mc_rung_mask(int nchain, int ntemp, int r) {
  unsigned long long m = 0ull;
  for (int j = r; j < nchain; j += ntemp) m |= 1ull << j;
  return m;
}

// the box of knot k of inner cell `cell`
struct McBox { double lo, hi; };
__device__ __forceinline__ McBox mc_box(const McDev &M, int cell, int k) {
  const long o = (long)k * M.ncell + cell;
  return {(double)M.vmin[o], (double)M.vmax[o]};
}

// the four standard normals of Philox block 1 + q of chain gid at `step`, knots 4 q .. 4 q + 3 (Box-Muller, two pairs; block 0
// decides and swaps)
struct McNormals { double z[4]; };
__device__ __forceinline__ McNormals mc_normals(const McDev &M, long long step, unsigned gid, int q) {
  unsigned w[4];
  mc_block(w, step, gid, 1u + (unsigned)q, M.seed);
  const double r0 = sqrt(-2.0 * log(mc_uniform(w[0]))), t0 = 6.283185307179586 * mc_uniform(w[1]);
  const double r1 = sqrt(-2.0 * log(mc_uniform(w[2]))), t1 = 6.283185307179586 * mc_uniform(w[3]);
  return {{r0 * cos(t0), r0 * sin(t0), r1 * cos(t1), r1 * sin(t1)}};
}

// knot k of the next proposal of column col: v' = v + s (vmax - vmin) y in fp64, reflected into the box, fp32.  RAD (a radial
// handle): a Vsv knot goes to the Vsv model too, which the Rayleigh curves of dazim_mc_run are computed from
template <int RAD>
__device__ __forceinline__ void mc_store_proposal(const McDev &M, int cell, long col, int k, float s, double y) {
  const McBox b = mc_box(M, cell, k);
  const double d = (double)s * (b.hi - b.lo);
  double v = (double)M.cur[k * M.ncol + col] + d * y;
  for (int r = 0; r < MC_MAXFOLD && (v < b.lo || v > b.hi); r++) v = v < b.lo ? 2.0 * b.lo - v : 2.0 * b.hi - v;
  const float vf = (float)fmin(fmax(v, b.lo), b.hi);
  M.prop[k * M.ncol + col] = vf;
  if constexpr (RAD) {
    if (k < M.nrad) M.vsv[k * M.ncol + col] = vf;
  }
}

// the next proposal of chain (cs, ch) from its current state, isotropic in box units: y = z
template <int RAD>
__device__ void mc_propose(const McDev &M, int cs, int ch, long long step, float s) {
  const int cell = M.cell_of[cs];
  const long col = (long)cs * M.nchain + ch;
  const unsigned gid = (unsigned)((long)cell * M.nchain + ch);
  for (int q = 0; q * 4 < M.nlay; q++) {
    const McNormals n = mc_normals(M, step, gid, q);
    for (int i = 0; i < 4 && q * 4 + i < M.nlay; i++) mc_store_proposal<RAD>(M, cell, col, q * 4 + i, s, n.z[i]);
  }
}

// the step scale at the end of an adaptation window: win accepted moves of ndec decisions (nadapt steps of the chains that share the
// scale); a cell with a factor (kind 1) may go up to 2 / sqrt(nlay)
__device__ __forceinline__ float mc_adapt_scale(float s, int win, double ndec, bool factor, int nlay) {
  const double rate = (double)win / ndec;
  if (rate > 0.40) s = s * 1.25f;
  else if (rate < 0.20) s = s / 1.25f;
  const float smax = factor ? 2.0f / sqrtf((float)nlay) : MC_SMAX;
  return fminf(fmaxf(s, MC_SMIN), smax);
}

// packed pair e = a (a + 1) / 2 + c, c <= a
__device__ __forceinline__ void mc_pair(int e, int &a, int &c) {
  a = 0;
  while ((a + 1) * (a + 2) / 2 <= e) a++;
  c = e - a * (a + 1) / 2;
}

// kind 1, a burn-in step with a decision: the cell's states us [nlay][nchain] (LDS) join the sums, pair e on lane e mod 64, the
// chains in chain order inside the lane; the lane of the diagonal pair (a, a) keeps s1[a] too.  Tempered handles pass stride =
// ntemp: the rung-0 chains alone
__device__ void mc_cov_accumulate(const McDev &M, int cs, int ch, const float *us, int stride) {
  const int n = M.nlay, npair = n * (n + 1) / 2, nc = M.nchain, cell = M.cell_of[cs];
  double *s1 = M.cov_s1 + (long)cs * n, *s2 = M.cov_s2 + (long)cs * npair;
  for (int e = ch; e < npair; e += MC_WAVE) {
    int a, c;
    mc_pair(e, a, c);
    const McBox ba = mc_box(M, cell, a), bc = mc_box(M, cell, c);
    const double wa = ba.hi - ba.lo, wc = bc.hi - bc.lo;
    double t1 = a == c ? s1[a] : 0.0, t2 = s2[e];
    for (int j = 0; j < nc; j += stride) {
      const double ua = ((double)us[a * nc + j] - ba.lo) / wa, uc = ((double)us[c * nc + j] - bc.lo) / wc;
      t1 += ua;
      t2 += ua * uc;
    }
    s2[e] = t2;
    if (a == c) s1[a] = t1;
  }
  if (ch == 0) M.cov_n[cs] += nc / stride;
}

// kind 1, an adaptation point with cn >= MC_COV_MIN nlay states in the sums (visible to every lane): the covariance of the window
// into L (LDS, packed lower triangle), the sums back to 0, then k_column_lsq's right-looking Cholesky on the packed triangle.
// Returns whether every pivot was finite and > 0 (the same on every lane); L holds the factor then.
__device__ bool mc_cov_factor(const McDev &M, int cs, int ch, long long cn, double *L) {
  const int n = M.nlay, npair = n * (n + 1) / 2;
  double *s1 = M.cov_s1 + (long)cs * n, *s2 = M.cov_s2 + (long)cs * npair;
  const double dn = (double)cn;
  for (int e = ch; e < npair; e += MC_WAVE) {
    int a, c;
    mc_pair(e, a, c);
    double C = s2[e] / dn - (s1[a] / dn) * (s1[c] / dn);
    if (a == c) C += MC_COV_RIDGE;
    L[e] = C;
  }
  __syncthreads();
  for (int e = ch; e < npair; e += MC_WAVE) s2[e] = 0.0;
  if (ch < n) s1[ch] = 0.0;
  if (ch == 0) M.cov_n[cs] = 0;
  for (int c = 0; c < n; c++) {                   // column c
    const int cc = c * (c + 1) / 2 + c;
    const double p = L[cc];
    if (!(isfinite(p) && p > 0.0)) return false;
    const double d = sqrt(p);
    if (ch > c && ch < n) L[ch * (ch + 1) / 2 + c] /= d;
    __syncthreads();
    if (ch == c) L[cc] = d;
    const int m = n - c - 1;
    for (int q = ch; q < m * m; q += MC_WAVE) {
      const int a = c + 1 + q / m, e = c + 1 + q % m;
      if (e <= a) L[a * (a + 1) / 2 + e] -= L[a * (a + 1) / 2 + c] * L[e * (e + 1) / 2 + c];
    }
    __syncthreads();
  }
  return true;
}

// kind 1, a cell with a factor: v' = v + s (vmax - vmin) y, y = L z with the normals of mc_propose, y_k summed in j order in fp64.
// zs [nlay][nchain] (LDS) takes the chain's normals; L is read at one address by every lane (a broadcast).
template <int RAD>
__device__ void mc_propose_cov(const McDev &M, int cs, int ch, long long step, float s, const double *L, double *zs) {
  const int cell = M.cell_of[cs], nc = M.nchain;
  const long col = (long)cs * M.nchain + ch;
  const unsigned gid = (unsigned)((long)cell * M.nchain + ch);
  for (int q = 0; q * 4 < M.nlay; q++) {
    const McNormals n = mc_normals(M, step, gid, q);
    for (int i = 0; i < 4 && q * 4 + i < M.nlay; i++) zs[(q * 4 + i) * nc + ch] = n.z[i];
  }
  for (int k = 0; k < M.nlay; k++) {
    const double *Lk = L + k * (k + 1) / 2;
    double y = 0.0;
    for (int j = 0; j <= k; j++) y += Lk[j] * zs[j * nc + ch];
    mc_store_proposal<RAD>(M, cell, col, k, s, y);
  }
}

// one wavefront per sampled cell, lane = chain: the start models (step 0 of the counter), the fixed last knot, the bookkeeping
__global__ __launch_bounds__(MC_WAVE) void k_mc_init(McDev M, float step0) {
  const int cs = blockIdx.x, ch = threadIdx.x;
  if (ch >= M.nchain) return;
  const int cell = M.cell_of[cs], nvx = M.nx - 2, j = cell / nvx, i = cell - j * nvx;
  const long col = (long)cs * M.nchain + ch, c0 = (long)(j + 1) * M.nx + (i + 1), nxy = (long)M.nx * M.ny;
  const unsigned gid = (unsigned)((long)cell * M.nchain + ch);
  for (int q = 0; q * 4 < M.nlay; q++) {
    unsigned w[4];
    mc_block(w, 0, gid, 1u + (unsigned)q, M.seed);
    for (int e = 0; e < 4 && q * 4 + e < M.nlay; e++) {
      const int k = q * 4 + e;
      const McBox b = mc_box(M, cell, k);
      const float v = (float)(b.lo + (b.hi - b.lo) * mc_uniform(w[e]));
      M.prop[k * M.ncol + col] = v;
      M.cur[k * M.ncol + col] = v;
    }
  }
  const float vl = M.vel0[(long)(M.nz - 1) * nxy + c0];
  M.prop[(long)(M.nz - 1) * M.ncol + col] = vl;
  M.cur[(long)(M.nz - 1) * M.ncol + col] = vl;
  M.chi2[col] = INFINITY;
  M.accepted[col] = 0;
  for (int k = 0; k < M.nlay; k++) {
    M.sums[(long)k * M.ncol + col] = 0.0;
    M.sums[((long)M.nlay + k) * M.ncol + col] = 0.0;
  }
  if (ch == 0) {
    M.scale[cs] = step0;
    M.acc_win[cs] = 0;
    M.best_chi2[cs] = INFINITY;
    for (int k = 0; k < M.nlay; k++) M.best[(long)k * M.ncs + cs] = M.vel0[(long)k * nxy + c0];
  }
}

// one step, one wavefront per sampled cell, lane = chain.  pv [kmax][ncol]: the curves of the proposals.
// first: the proposals are the start models -- they become the state, no decision.  adapt: the end of an adaptation window.
// KIND 1 (covariance proposals) adds, in dynamic LDS, L [npair] fp64 and behind it the normals zs [nlay][nchain] fp64, whose first
// half holds the staged states [nlay][nchain] fp32 while they are accumulated: 48 384 bytes at nlay = 63, nchain = 64.
// TEMPER 1 (a ladder of ntemp > 1 rungs): the decision of rung r takes beta_r, the scale and its window are per rung (lane r < ntemp
// keeps rung r's, counting its chains in the ballot), neighbouring rungs swap states by lane shuffles after the decision, and only
// the rung-0 lanes record.  Each lane carries its chi^2 in a register from the decision through the swap.
// NG >= 1 (noise scales, at most NG groups): the weight loop also forms chi^2_g and nd_g of every group (cgp, ndg), the decision and
// the swap compare mc_energy of two states, each lane carries the chi^2_g of its state (cgs) through the swap, whose rule compares
// the two lanes' own energies (a_g is the cell's, so the partner's value is the one this lane would form), the chi^2_g change lanes
// with the knots, and a recorded lane adds sqrt(B_g) and B_g per group with data to its own columns of nsum.  chi2 stays the total.
// PRIOR 1 (dazim_mc_set_prior): the lane walks its column of prop for Q', the decision and the swap compare energy + Q (mc_total; the
// rules for +inf still test chi^2 alone), Q travels beside chi^2 through the swap's shuffles, and pq keeps the Q of the lane's state.
// RAD 1 (dazim_mc_set_radial): Q is the stacked knots' (mc_prior_q_radial), a recorded lane adds xi, xi^2, vv vh, V, V^2 of every knot
// pair of its state to its own columns of rsum, counts xi > 1 there and xi into the cell's rhist, and a proposed Vsv knot goes to the
// Vsv model as well (mc_store_proposal).
template <int KIND, int TEMPER, int NG, int PRIOR, int RAD>
__global__ __launch_bounds__(MC_WAVE) void k_mc_step(McDev M, const double *__restrict__ pv, long long step, int first, int record,
                                                     int adapt, int nadapt) {
  __shared__ float s_scale;
  __shared__ int s_win;
  __shared__ float s_rscale[TEMPER ? MC_MAXCHAIN : 1];   // TEMPER: the scale of every rung
  const int cs = blockIdx.x, ch = threadIdx.x;
  const bool act = ch < M.nchain;
  const int cell = M.cell_of[cs];
  const long col = (long)cs * M.nchain + ch;
  const unsigned gid = (unsigned)((long)cell * M.nchain + ch);
  const int nt = TEMPER ? M.ntemp : 1, rung = ch % nt;
  double chi2p = 0.0;
  double chi2s = INFINITY;   // TEMPER: the chain's chi^2 after the decision, then after the swap
  unsigned wswap = 0u;       // TEMPER: word 1 of block(step, gid, 0), the swap uniform of a pair's lower chain
  double qp = 0.0, qs = 0.0;   // PRIOR: Q of the proposal; Q of the chain's state after the decision, then after the swap
  double cgp[NG ? NG : 1], cgs[NG ? NG : 1];   // NG: chi^2_g of the proposal; of the chain's state after the decision, then the swap
  int ndg[NG ? NG : 1];                        // ... the cell's periods with data per group
#pragma unroll
  for (int g = 0; g < (NG ? NG : 1); g++) {
    cgp[g] = 0.0;
    cgs[g] = INFINITY;
    ndg[g] = 0;
  }
  bool acc = false;
  if (act) {
    chi2p = mc_chi2<NG>(M, pv, cell, col, cgp, ndg);
    if constexpr (PRIOR) qp = RAD ? mc_prior_q_radial(M, M.prop, col, cell) : mc_prior_q(M, M.prop, col, cell);
    if (first) {
      acc = true;
    } else {
      // a chain without a curve takes the first proposal that has one; else Metropolis on the energies at the rung's beta (1 without
      // a ladder, which leaves the product's bits alone).  Where the first rule decides only a ladder draws block 0, for its word 1
      const double chi2c = M.chi2[col];
#pragma unroll
      for (int g = 0; g < NG; g++)
        if (mc_group_on<NG>(M, g)) cgs[g] = NG > 1 ? M.chi2g[(long)g * M.ncol + col] : chi2c;   // (one group's chi^2_g is chi^2)
      const double xp = mc_energy<NG>(M, ndg, cgp, chi2p), xc = mc_energy<NG>(M, ndg, cgs, chi2c);
      double beta = 1.0;
      if constexpr (TEMPER) beta = M.beta[rung];
      unsigned w[4] = {0u, 0u, 0u, 0u};
      if (TEMPER || !isinf(chi2c)) mc_block(w, step, gid, 0u, M.seed);
      wswap = w[1];
      chi2s = chi2c;
      if constexpr (PRIOR) qs = M.pq[col];
      acc = isinf(chi2c) ? !isinf(chi2p) : log(mc_uniform(w[0])) < -0.5 * beta * (mc_total<PRIOR>(xp, qp) - mc_total<PRIOR>(xc, qs));
    }
    if (acc) {
      for (int k = 0; k < M.nlay; k++) M.cur[k * M.ncol + col] = M.prop[k * M.ncol + col];
      M.chi2[col] = chi2p;
      chi2s = chi2p;
#pragma unroll
      for (int g = 0; g < NG; g++) {
        cgs[g] = cgp[g];
        if (NG > 1 && g < M.ngrp) M.chi2g[(long)g * M.ncol + col] = cgp[g];
      }
      if constexpr (PRIOR) {
        M.pq[col] = qp;
        qs = qp;
      }
    }
  }
  const unsigned long long bacc = first ? 0ull : __ballot(act && acc);
  const int nacc = __popcll(bacc);
  const int nnoroot = __popcll(__ballot(act && isinf(chi2p)));
  if constexpr (TEMPER) {
    // a swap round: pairs (r, r + 1), r of the round's parity, in every group; the pair's lower lane decides, both lanes take the
    // other's knots (each reads and writes its own column only) and chi^2
    if (!first && step % M.nswap == 0) {
      const int par = (int)((step / M.nswap) & 1);
      const bool lower = act && rung + 1 < nt && (rung & 1) == par;
      const bool upper = act && rung > 0 && ((rung - 1) & 1) == par;
      const double cup = __shfl_down(chi2s, 1), cdn = __shfl_up(chi2s, 1);
      double qup = 0.0, qdn = 0.0;
      if constexpr (PRIOR) {
        qup = __shfl_down(qs, 1);
        qdn = __shfl_up(qs, 1);
      }
      const double xs = mc_energy<NG>(M, ndg, cgs, chi2s), xup = __shfl_down(xs, 1);   // the lane's energy, the upper neighbour's
      int sw = 0;
      if (lower) {
        if (isinf(chi2s)) sw = !isinf(cup);
        else if (!isinf(cup))
          sw = log(mc_uniform(wswap)) < 0.5 * (M.beta[rung] - M.beta[rung + 1]) * (mc_total<PRIOR>(xs, qs) - mc_total<PRIOR>(xup, qup));
      }
      const int swu = __shfl_up(sw, 1);
      const bool swp = lower ? sw != 0 : (upper && swu != 0);
      const int partner = lower ? ch + 1 : (upper ? ch - 1 : ch);
      for (int k = 0; k < M.nlay; k++) {
        const float v = act ? M.cur[k * M.ncol + col] : 0.0f;
        const float vp = __shfl(v, partner);
        if (swp) M.cur[k * M.ncol + col] = vp;
      }
#pragma unroll
      for (int g = 0; g < NG; g++) {
        const double cp = __shfl(cgs[g], partner);
        if (swp) {
          cgs[g] = cp;
          if (NG > 1 && g < M.ngrp) M.chi2g[(long)g * M.ncol + col] = cp;
        }
      }
      if (swp) {
        chi2s = lower ? cup : cdn;
        M.chi2[col] = chi2s;
        if constexpr (PRIOR) {
          qs = lower ? qup : qdn;
          M.pq[col] = qs;
        }
      }
      const unsigned long long btry = __ballot(lower), bswp = __ballot(lower && sw != 0);
      if (ch < nt - 1) {
        const unsigned long long mask = mc_rung_mask(M.nchain, nt, ch);
        M.swap_try[(long)cs * (nt - 1) + ch] += __popcll(btry & mask);
        M.swap_acc[(long)cs * (nt - 1) + ch] += __popcll(bswp & mask);
      }
    }
  }
  if (ch == 0 && nnoroot) atomicAdd(&M.counters[0], (unsigned long long)nnoroot);
  if (ch < nt) {   // lane r keeps rung r's scale and window: the ladder's, or without one lane 0 the cell's own
    const int nar = TEMPER ? __popcll(bacc & mc_rung_mask(M.nchain, nt, ch)) : nacc;
    const long o = (long)cs * nt + ch;
    float *sc = TEMPER ? M.tscale + o : M.scale + o;
    int *wn = TEMPER ? M.tacc_win + o : M.acc_win + o;
    float s = *sc;
    if (!record) {
      int win = *wn + nar;
      if (adapt) {
        s = mc_adapt_scale(s, win, (double)nadapt * (double)(M.nchain / nt), KIND == 1 && M.cov_set[cs], M.nlay);
        *sc = s;
        if (TEMPER && ch == 0) M.scale[cs] = s;
        win = 0;
      }
      *wn = win;
    } else if (ch == 0 && nar) {
      atomicAdd(&M.counters[1], (unsigned long long)nar);
    }
    (TEMPER ? s_rscale[ch] : s_scale) = s;
  }
  if (record) {
    if (act && rung == 0) {
      if (!first && acc) M.accepted[col] += 1;
      for (int k = 0; k < M.nlay; k++) {
        const double v = (double)M.cur[k * M.ncol + col];
        M.sums[(long)k * M.ncol + col] += v;
        M.sums[((long)M.nlay + k) * M.ncol + col] += v * v;
        const McBox bx = mc_box(M, cell, k);
        int b = (int)((v - bx.lo) / (bx.hi - bx.lo) * (double)M.nbin);
        b = b < 0 ? 0 : (b >= M.nbin ? M.nbin - 1 : b);
        atomicAdd(&M.hist[((long)cs * M.nlay + k) * M.nbin + b], 1u);
      }
      if constexpr (RAD) {
        const int n = M.nrad;
        const long nn = (long)n * M.ncol;
        for (int a = 0; a < n; a++) {
          const double vv = (double)M.cur[a * M.ncol + col], vh = (double)M.cur[(n + a) * M.ncol + col];
          const double r = vh / vv, xi = r * r, V = sqrt((2.0 * vv * vv + vh * vh) / 3.0);
          const long o = (long)a * M.ncol + col;
          M.rsum[o] += xi;
          M.rsum[nn + o] += xi * xi;
          M.rsum[2 * nn + o] += vv * vh;
          M.rsum[3 * nn + o] += V;
          M.rsum[4 * nn + o] += V * V;
          if (xi > 1.0) M.rgt1[o] += 1;
          const McBox bv = mc_box(M, cell, a), bh = mc_box(M, cell, n + a);
          const double rl = bh.lo / bv.hi, rh = bh.hi / bv.lo, xlo = rl * rl, xhi = rh * rh;
          int b = (int)((xi - xlo) / (xhi - xlo) * (double)M.nbin);
          b = b < 0 ? 0 : (b >= M.nbin ? M.nbin - 1 : b);
          atomicAdd(&M.rhist[((long)cs * n + a) * M.nbin + b], 1u);
        }
      }
      if constexpr (NG >= 1) {
        if (!isinf(M.chi2[col])) {   // (cgs: the state's chi^2_g, after the decision and the swap)
#pragma unroll
          for (int g = 0; g < NG; g++)
            if (mc_group_on<NG>(M, g) && ndg[g] > 0) {
              const double B = (double)M.gb0[g] + 0.5 * cgs[g];
              M.nsum[(long)g * M.ncol + col] += sqrt(B);
              M.nsum[((long)M.ngrp + g) * M.ncol + col] += B;
            }
          M.ncnt[col] += 1;
        }
      }
    }
    // the lowest chi^2 of this step, the first chain on ties; it replaces the cell's best only when strictly lower
    double m = act ? M.chi2[col] : INFINITY;
    int l = ch;
    for (int o = 32; o > 0; o >>= 1) {
      const double m2 = __shfl_xor(m, o);
      const int l2 = __shfl_xor(l, o);
      if (m2 < m || (m2 == m && l2 < l)) {
        m = m2;
        l = l2;
      }
    }
    if (ch == 0) s_win = m < M.best_chi2[cs] ? l : -1;
    __syncthreads();
    const int win = s_win;
    if (win >= 0) {
      if (ch < M.nlay) M.best[(long)ch * M.ncs + cs] = M.cur[(long)ch * M.ncol + (long)cs * M.nchain + win];
      if (ch == 0) M.best_chi2[cs] = m;
    }
  }
  if constexpr (KIND == 1) {
    extern __shared__ double mc_lds[];
    const int npair = M.nlay * (M.nlay + 1) / 2;
    double *L = mc_lds, *zs = mc_lds + npair;
    int set = M.cov_set[cs];
    bool have = false;   // L holds the cell's factor
    if (!record && !first) {
      float *us = (float *)zs;
      if (act)
        for (int k = 0; k < M.nlay; k++) us[k * M.nchain + ch] = M.cur[k * M.ncol + col];
      __syncthreads();
      mc_cov_accumulate(M, cs, ch, us, nt);
      if (adapt) {
        __syncthreads();
        const long long cn = M.cov_n[cs];
        if (cn >= (long long)MC_COV_MIN * M.nlay && mc_cov_factor(M, cs, ch, cn, L)) {
          for (int e = ch; e < npair; e += MC_WAVE) M.chol[(long)cs * npair + e] = L[e];
          have = true;
          if (!set) {   // the first factor: the scale restarts for the new metric
            set = 1;
            if constexpr (TEMPER) {
              if (ch < nt) {
                s_rscale[ch] = 1.0f / sqrtf((float)M.nlay);
                M.tscale[(long)cs * nt + ch] = s_rscale[ch];
              }
            }
            if (ch == 0) {
              M.cov_set[cs] = 1;
              s_scale = 1.0f / sqrtf((float)M.nlay);
              M.scale[cs] = s_scale;
            }
          }
        }
      }
    }
    __syncthreads();
    const float s = TEMPER ? s_rscale[rung] : s_scale;
    if (set) {
      if (!have)
        for (int e = ch; e < npair; e += MC_WAVE) L[e] = M.chol[(long)cs * npair + e];
      __syncthreads();
      if (act) mc_propose_cov<RAD>(M, cs, ch, step, s, L, zs);
    } else if (act) {
      mc_propose<RAD>(M, cs, ch, step, s);
    }
  } else {
    __syncthreads();
    if (act) mc_propose<RAD>(M, cs, ch, step, TEMPER ? s_rscale[rung] : s_scale);
  }
}

// posterior statistics, one wavefront per inner cell, lane = knot.  nrec: recorded steps; ndec: recorded steps with a decision.
// The recorded chains are ch = 0, ntemp, 2 ntemp, .. (every chain without tempering), M of them
__global__ __launch_bounds__(MC_WAVE) void k_mc_final(McDev M, long long nrec, long long ndec, float *__restrict__ mean,
                                                      float *__restrict__ stdv, float *__restrict__ q, float *__restrict__ best,
                                                      float *__restrict__ rhat, float *__restrict__ accept, float *__restrict__ chi2_best) {
  const int cell = blockIdx.x, k = threadIdx.x;
  const int cs = M.cs_of[cell], nvx = M.nx - 2, j = cell / nvx, i = cell - j * nvx;
  const long c0 = (long)(j + 1) * M.nx + (i + 1), nxy = (long)M.nx * M.ny, o = (long)k * M.ncell + cell;
  if (cs < 0) {   // no data: the start model
    if (k < M.nlay) {
      const float v = M.vel0[(long)k * nxy + c0];
      mean[o] = v;
      stdv[o] = 0.0f;
      best[o] = v;
      rhat[o] = NAN;
      for (int e = 0; e < 3; e++) q[(long)e * M.nlay * M.ncell + o] = v;
    }
    if (k == 0) {
      accept[cell] = 0.0f;
      chi2_best[cell] = 0.0f;
    }
    return;
  }
  if (k < M.nlay) {
    const double N = (double)nrec, Mc = (double)(M.nchain / M.ntemp);
    double s1 = 0.0, s2 = 0.0, sm = 0.0;
    for (int ch = 0; ch < M.nchain; ch += M.ntemp) {
      const long col = (long)cs * M.nchain + ch;
      const double a = M.sums[(long)k * M.ncol + col], b = M.sums[((long)M.nlay + k) * M.ncol + col];
      s1 += a;
      s2 += b;
      sm += a / N;
    }
    const double mu = s1 / (N * Mc);
    mean[o] = (float)mu;
    stdv[o] = (float)sqrt(fmax(s2 / (N * Mc) - mu * mu, 0.0));
    // R-hat (BDA3, chains not split): W the mean within-chain variance, B / N the variance of the chain means
    double W = 0.0, B = 0.0;
    const double mbar = sm / Mc;
    for (int ch = 0; ch < M.nchain; ch += M.ntemp) {
      const long col = (long)cs * M.nchain + ch;
      const double a = M.sums[(long)k * M.ncol + col], b = M.sums[((long)M.nlay + k) * M.ncol + col];
      const double mj = a / N;
      W += (b - N * mj * mj) / (N - 1.0);
      B += (mj - mbar) * (mj - mbar);
    }
    W /= Mc;
    B *= N / (Mc - 1.0);
    rhat[o] = (M.nchain / M.ntemp > 1 && nrec > 1 && W > 0.0) ? (float)sqrt(((N - 1.0) / N * W + B / N) / W) : NAN;
    // 2.5 / 50 / 97.5 % from the counts, linear inside a bin
    const unsigned *h = M.hist + ((long)cs * M.nlay + k) * M.nbin;
    const double lo = (double)M.vmin[o], hi = (double)M.vmax[o], tot = N * Mc;
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
      q[(long)e * M.nlay * M.ncell + o] = (float)(lo + pos * (hi - lo) / (double)M.nbin);
    }
    best[o] = M.best[(long)k * M.ncs + cs];
  }
  if (k == 0) {
    long long a = 0;
    for (int ch = 0; ch < M.nchain; ch += M.ntemp) a += M.accepted[(long)cs * M.nchain + ch];
    accept[cell] = ndec > 0 ? (float)((double)a / ((double)ndec * (double)(M.nchain / M.ntemp))) : 0.0f;
    chi2_best[cell] = (float)M.best_chi2[cs];
  }
}

// the noise scales' posteriors (dazim_mc_noise_result, dazim_mc_noise_groups_result), one lane per (group, inner cell): conditional on
// a state lambda_g^2 ~ IG(a_g, B_g), so E[lambda_g] = g(a_g) E[sqrt(B_g)] and E[lambda_g^2] = E[B_g] / (a_g - 1); the cell's cold
// columns in column order inside the lane, the record's count the cell's; 0 for a group without data in the cell
__global__ __launch_bounds__(MC_WAVE) void k_mc_noise_final(McDev M, float *__restrict__ lam_mean, float *__restrict__ lam_std,
                                                            int *__restrict__ ndata) {
  const long i = (long)blockIdx.x * MC_WAVE + threadIdx.x;
  if (i >= (long)M.ngrp * M.ncell) return;
  const int g = (int)(i / M.ncell), cell = (int)(i - (long)g * M.ncell);
  const int cs = M.cs_of[cell];
  int nd = 0;
  for (int p = 0; p < M.kmax; p++) nd += M.grp[p] == g && M.wdat[(long)p * M.ncell + cell] != 0.0f;
  ndata[i] = nd;
  if (cs < 0 || nd == 0) {
    lam_mean[i] = 0.0f;
    lam_std[i] = 0.0f;
    return;
  }
  long long n = 0;
  double s0 = 0.0, s1 = 0.0;
  for (int ch = 0; ch < M.nchain; ch += M.ntemp) {
    const long col = (long)cs * M.nchain + ch;
    n += M.ncnt[col];
    s0 += M.nsum[(long)g * M.ncol + col];
    s1 += M.nsum[((long)M.ngrp + g) * M.ncol + col];
  }
  if (n == 0) {
    lam_mean[i] = NAN;
    lam_std[i] = NAN;
    return;
  }
  float a0 = 0.0f;
#pragma unroll
  for (int q = 0; q < MC_MAXGRP; q++)
    if (q == g) a0 = M.ga0[q];
  const double a = (double)a0 + 0.5 * nd, dn = (double)n;
  const double lm = M.ngam[g * (MC_MAXPER + 1) + nd] * s0 / dn;
  lam_mean[i] = (float)lm;
  lam_std[i] = a <= 1.0 ? NAN : (float)sqrt(fmax(s1 / (dn * (a - 1.0)) - lm * lm, 0.0));
}

// the step kernel of a handle: [radial][prior][noise: off, one group, more][kind][tempered]
using McStepKernel = void (*)(McDev, const double *, long long, int, int, int, int);
#define MC_STEP_NG(G, P, R) {{k_mc_step<0, 0, G, P, R>, k_mc_step<0, 1, G, P, R>}, {k_mc_step<1, 0, G, P, R>, k_mc_step<1, 1, G, P, R>}}
#define MC_STEP_SET(P, R) {MC_STEP_NG(0, P, R), MC_STEP_NG(1, P, R), MC_STEP_NG(MC_MAXGRP, P, R)}
constexpr McStepKernel MC_STEP[2][2][3][2][2] = {{MC_STEP_SET(0, 0), MC_STEP_SET(1, 0)}, {MC_STEP_SET(0, 1), MC_STEP_SET(1, 1)}};
#undef MC_STEP_SET
#undef MC_STEP_NG

// the Q of every chain's state into pq (dazim_mc_set_prior; the step keeps it from there on), lane = chain
__global__ __launch_bounds__(MC_WAVE) void k_mc_prior_q(McDev M) {
  const int cs = blockIdx.x, ch = threadIdx.x;
  if (ch >= M.nchain) return;
  const long col = (long)cs * M.nchain + ch;
  M.pq[col] = M.nrad ? mc_prior_q_radial(M, M.cur, col, M.cell_of[cs]) : mc_prior_q(M, M.cur, col, M.cell_of[cs]);
}

// one step on the curves pv (device) of the current proposals; enqueued on the ctx stream, no host wait
// vel0's knots at the inner cells [nlay][ncell]: the prior's centre where the caller names none
int mc_vel0_knots(dazim_ctx *ctx, dazim_mc *mc, std::vector<float> &knots) {
  const McDev &M = mc->d;
  std::vector<float> vel0;
  int rc;
  if ((rc = mc_to_host(ctx, M.vel0, (size_t)M.nz * M.nx * M.ny, vel0))) return rc;
  knots.resize((size_t)M.nlay * M.ncell);
  const int nvx = M.nx - 2;
  for (int k = 0; k < M.nlay; k++)
    for (int c = 0; c < M.ncell; c++) knots[(size_t)k * M.ncell + c] = vel0[((size_t)k * M.ny + (c / nvx + 1)) * M.nx + (c % nvx + 1)];
  return 0;
}

int mc_launch_step(dazim_ctx *ctx, dazim_mc *mc, const double *pv, int record) {
  const bool first = mc->nstep == 0;
  bool adapt = false;
  if (!record && !first) {
    mc->nburn_dec++;
    adapt = mc->nburn_dec % mc->nadapt == 0;
  }
  const long long step = mc->nstep + 1;
  if (mc->d.ncs > 0) {
    DZ_HIP(hipEventRecord(mc->e0, ctx->stream));
    const size_t lds =
        mc->kind == 1 ? ((size_t)mc->d.nlay * (mc->d.nlay + 1) / 2 + (size_t)mc->d.nlay * mc->d.nchain) * sizeof(double) : 0;
    const McStepKernel kern = MC_STEP[mc->d.nrad > 0][mc->prior][std::min(mc->d.ngrp, 2)][mc->kind][mc->d.ntemp > 1];
    hipLaunchKernelGGL(kern, dim3((unsigned)mc->d.ncs), dim3(MC_WAVE), lds, ctx->stream, mc->d, pv, step, (int)first, record, (int)adapt,
                       mc->nadapt);
    DZ_HIP(hipGetLastError());
    DZ_HIP(hipEventRecord(mc->e1, ctx->stream));
  }
  mc->nstep = step;
  if (record) {
    mc->nrec++;
    if (!first) mc->nrec_dec++;
  }
  return 0;
}
}  // namespace

int mc_prior_refresh(dazim_ctx *ctx, dazim_mc *mc, const std::vector<float> *vref) {
  McDev &M = mc->d;
  if (mc->psmooth == 0.0f && mc->pdamp == 0.0f && !(M.nrad > 0 && mc->couple != 0.0f)) {
    mc->prior = 0;
    return 0;
  }
  DZ_HIP(hipSetDevice(ctx->device));
  int rc;
  const size_t nk = (size_t)M.nlay * M.ncell;
  std::vector<float> knots;
  if (!vref && !M.pref) {
    if ((rc = mc_vel0_knots(ctx, mc, knots))) return rc;
    vref = &knots;
  }
  if (!M.pq) {
    float *r;
    if ((rc = mc_alloc(mc, nk, &r)) || (rc = mc_alloc(mc, (size_t)M.ncol, &M.pq))) return rc;
    M.pref = r;
  }
  if (vref) DZ_HIP(hipMemcpyAsync((void *)M.pref, vref->data(), nk * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (M.ncs > 0) {   // the start models are the states until the first step
    hipLaunchKernelGGL(k_mc_prior_q, dim3((unsigned)M.ncs), dim3(MC_WAVE), 0, ctx->stream, M);
    DZ_HIP(hipGetLastError());
  }
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  mc->prior = 1;
  return 0;
}

extern "C" {

int dazim_mc_create(dazim_ctx *ctx, int nx, int ny, int nz, int kmax, int nchain, int nbin, unsigned long long seed, const float *vel0_u,
                    const float *vmin_u, const float *vmax_u, const float *cobs_u, const float *wdat_u, float step, int nadapt,
                    dazim_mc **out, int *n_empty) {
  if (!ctx || !out || !vel0_u || !vmin_u || !vmax_u || !cobs_u || !wdat_u || nx < 3 || ny < 3)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_create");
  *out = nullptr;
  const int nlay = nz - 1;
  if (nlay < 1 || nlay > MC_MAXLAY) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: nlay %d outside 1..%d", nlay, MC_MAXLAY);
  if (kmax < 1 || kmax > MC_MAXPER) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: kmax %d outside 1..%d", kmax, MC_MAXPER);
  if (nchain < 1 || nchain > MC_MAXCHAIN)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: nchain %d outside 1..%d", nchain, MC_MAXCHAIN);
  if (nbin < 2) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: nbin %d < 2", nbin);
  if (!(step > 0.0f && step <= MC_SMAX)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: step %g outside (0, %g]", step, MC_SMAX);
  if (nadapt < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: nadapt %d < 1", nadapt);
  DZ_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (nx - 2) * (ny - 2);
  std::vector<float> vel0, vmin, vmax, cobs, wdat;
  if ((rc = mc_to_host(ctx, vel0_u, (size_t)nz * nx * ny, vel0)) || (rc = mc_to_host(ctx, vmin_u, (size_t)nlay * ncell, vmin)) ||
      (rc = mc_to_host(ctx, vmax_u, (size_t)nlay * ncell, vmax)) || (rc = mc_to_host(ctx, cobs_u, (size_t)kmax * ncell, cobs)) ||
      (rc = mc_to_host(ctx, wdat_u, (size_t)kmax * ncell, wdat)))
    return rc;
  for (size_t e = 0; e < vmin.size(); e++)
    if (!std::isfinite(vmin[e]) || !std::isfinite(vmax[e]))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: a non-finite bound at knot %d, cell %d", (int)(e / ncell), (int)(e % ncell));
    else if (!(vmin[e] < vmax[e]))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: vmin %g >= vmax %g at knot %d, cell %d", vmin[e], vmax[e],
                     (int)(e / ncell), (int)(e % ncell));
  for (size_t e = 0; e < cobs.size(); e++)
    if (!std::isfinite(cobs[e]) || !std::isfinite(wdat[e]))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_create: a non-finite cobs or wdat at period %d, cell %d", (int)(e / ncell),
                     (int)(e % ncell));
  std::vector<int> cell_of, cs_of(ncell, -1);
  for (int c = 0; c < ncell; c++) {
    bool data = false;
    for (int p = 0; p < kmax; p++) data = data || wdat[(size_t)p * ncell + c] != 0.0f;
    if (data) {
      cs_of[c] = (int)cell_of.size();
      cell_of.push_back(c);
    }
  }
  dazim_mc *mc = new dazim_mc();
  mc->ctx = ctx;
  mc->nadapt = nadapt;
  mc->step0 = step;
  mc->n_empty = ncell - (int)cell_of.size();
  McDev &M = mc->d;
  M.nx = nx;
  M.ny = ny;
  M.nz = nz;
  M.nlay = nlay;
  M.kmax = kmax;
  M.nchain = nchain;
  M.nbin = nbin;
  M.ncell = ncell;
  M.ncs = (int)cell_of.size();
  M.ncol = (long)M.ncs * nchain;
  M.seed = seed;
  M.ntemp = 1;
  M.nswap = 1;
  int *ci, *co;
  float *v0, *lo, *hi, *co_, *wd;
  const auto fail = [&](int r) { mc_release(mc); return r; };
  if ((rc = mc_alloc(mc, cell_of.size(), &ci)) || (rc = mc_alloc(mc, (size_t)ncell, &co)) || (rc = mc_alloc(mc, vel0.size(), &v0)) ||
      (rc = mc_alloc(mc, vmin.size(), &lo)) || (rc = mc_alloc(mc, vmax.size(), &hi)) || (rc = mc_alloc(mc, cobs.size(), &co_)) ||
      (rc = mc_alloc(mc, wdat.size(), &wd)) || (rc = mc_alloc(mc, (size_t)nz * M.ncol, &M.cur)) ||
      (rc = mc_alloc(mc, (size_t)nz * M.ncol, &M.prop)) || (rc = mc_alloc(mc, (size_t)M.ncol, &M.chi2)) ||
      (rc = mc_alloc(mc, (size_t)M.ncs, &M.scale)) || (rc = mc_alloc(mc, (size_t)M.ncs, &M.acc_win)) ||
      (rc = mc_alloc(mc, (size_t)2 * nlay * M.ncol, &M.sums)) || (rc = mc_alloc(mc, (size_t)M.ncs * nlay * nbin, &M.hist)) ||
      (rc = mc_alloc(mc, (size_t)M.ncol, &M.accepted)) || (rc = mc_alloc(mc, (size_t)nlay * M.ncs, &M.best)) ||
      (rc = mc_alloc(mc, (size_t)M.ncs, &M.best_chi2)) || (rc = mc_alloc(mc, (size_t)2, &M.counters)) ||
      (rc = mc_alloc(mc, (size_t)kmax * M.ncol, &mc->pv)))
    return fail(rc);
  M.cell_of = ci;
  M.cs_of = co;
  M.vel0 = v0;
  M.vmin = lo;
  M.vmax = hi;
  M.cobs = co_;
  M.wdat = wd;
  auto up = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
  };
  const auto start = [&]() -> hipError_t {   // the tables, the events, the start models
    hipError_t e;
    if ((e = up(ci, cell_of.data(), cell_of.size() * 4)) != hipSuccess || (e = up(co, cs_of.data(), cs_of.size() * 4)) != hipSuccess ||
        (e = up(v0, vel0.data(), vel0.size() * 4)) != hipSuccess || (e = up(lo, vmin.data(), vmin.size() * 4)) != hipSuccess ||
        (e = up(hi, vmax.data(), vmax.size() * 4)) != hipSuccess || (e = up(co_, cobs.data(), cobs.size() * 4)) != hipSuccess ||
        (e = up(wd, wdat.data(), wdat.size() * 4)) != hipSuccess ||
        (e = hipMemsetAsync(M.hist, 0, (size_t)M.ncs * nlay * nbin * sizeof(unsigned), ctx->stream)) != hipSuccess ||
        (e = hipMemsetAsync(M.counters, 0, 16, ctx->stream)) != hipSuccess || (e = hipEventCreate(&mc->e0)) != hipSuccess ||
        (e = hipEventCreate(&mc->e1)) != hipSuccess)
      return e;
    if (M.ncs > 0) {
      hipLaunchKernelGGL(k_mc_init, dim3((unsigned)M.ncs), dim3(MC_WAVE), 0, ctx->stream, M, step);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipStreamSynchronize(ctx->stream);
  };
  const hipError_t e = start();
  if (e != hipSuccess) return fail(dz_fail(ctx, -(int)e - 1000, "dazim_mc_create: %s", hipGetErrorString(e)));
  *out = mc;
  if (n_empty) *n_empty = mc->n_empty;
  return 0;
}

int dazim_mc_proposals(dazim_mc *mc, float **vel_dev, int64_t *ncol) {
  if (!mc) return DAZIM_E_BAD_ARG;
  if (vel_dev) *vel_dev = mc->d.prop;
  if (ncol) *ncol = mc->d.ncol;
  return 0;
}

int dazim_mc_set_proposal(dazim_ctx *ctx, dazim_mc *mc, int kind) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_set_proposal"))) return rc;
  if (kind != 0 && kind != 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_proposal: kind %d is neither 0 nor 1", kind);
  if (mc->nstep > 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_proposal: the handle has done %lld steps", (long long)mc->nstep);
  DZ_HIP(hipSetDevice(ctx->device));
  McDev &M = mc->d;
  if (kind == 1 && !M.chol) {
    const size_t n1 = (size_t)M.ncs * M.nlay, n2 = (size_t)M.ncs * (M.nlay * (M.nlay + 1) / 2);
    if ((rc = mc_alloc(mc, (size_t)M.ncs, &M.cov_n)) || (rc = mc_alloc(mc, n1, &M.cov_s1)) || (rc = mc_alloc(mc, n2, &M.cov_s2)) ||
        (rc = mc_alloc(mc, (size_t)M.ncs, &M.cov_set)) || (rc = mc_alloc(mc, n2, &M.chol)))
      return rc;
    DZ_HIP(hipMemsetAsync(M.cov_n, 0, (size_t)M.ncs * sizeof(long long), ctx->stream));
    DZ_HIP(hipMemsetAsync(M.cov_s1, 0, n1 * sizeof(double), ctx->stream));
    DZ_HIP(hipMemsetAsync(M.cov_s2, 0, n2 * sizeof(double), ctx->stream));
    DZ_HIP(hipMemsetAsync(M.cov_set, 0, (size_t)M.ncs * sizeof(int), ctx->stream));
    DZ_HIP(hipMemsetAsync(M.chol, 0, n2 * sizeof(double), ctx->stream));
    DZ_HIP(hipStreamSynchronize(ctx->stream));
  }
  mc->kind = kind;
  return 0;
}

int dazim_mc_cov_state(dazim_ctx *ctx, dazim_mc *mc, int *kind, int64_t *cov_n, double *cov_s1, double *cov_s2, double *chol,
                       int *cov_set) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_cov_state"))) return rc;
  if (kind) *kind = mc->kind;
  if (mc->kind != 1) {
    if (cov_n || cov_s1 || cov_s2 || chol || cov_set)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_cov_state: the handle's proposal kind %d keeps no covariance", mc->kind);
    return 0;
  }
  DZ_HIP(hipSetDevice(ctx->device));
  const McDev &M = mc->d;
  const size_t n1 = (size_t)M.ncs * M.nlay, n2 = (size_t)M.ncs * (M.nlay * (M.nlay + 1) / 2);
  DZ_HIP(mc_get(ctx, cov_n, M.cov_n, (size_t)M.ncs * 8));
  DZ_HIP(mc_get(ctx, cov_s1, M.cov_s1, n1 * 8));
  DZ_HIP(mc_get(ctx, cov_s2, M.cov_s2, n2 * 8));
  DZ_HIP(mc_get(ctx, chol, M.chol, n2 * 8));
  DZ_HIP(mc_get(ctx, cov_set, M.cov_set, (size_t)M.ncs * 4));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int dazim_mc_set_tempering(dazim_ctx *ctx, dazim_mc *mc, int ntemp, float tmax, int nswap) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_set_tempering"))) return rc;
  McDev &M = mc->d;
  if (ntemp < 1 || ntemp > M.nchain || M.nchain % ntemp != 0)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_tempering: ntemp %d does not divide the %d chains", ntemp, M.nchain);
  if (ntemp > 1 && !(std::isfinite(tmax) && tmax > 1.0f))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_tempering: tmax %g is not a finite temperature above 1", tmax);
  if (nswap < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_tempering: nswap %d < 1", nswap);
  if (mc->nstep > 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_tempering: the handle has done %lld steps", (long long)mc->nstep);
  DZ_HIP(hipSetDevice(ctx->device));
  std::vector<double> beta((size_t)ntemp, 1.0);
  for (int r = 1; r < ntemp; r++) beta[r] = std::pow((double)tmax, -(double)r / (double)(ntemp - 1));
  if (ntemp > 1) {
    // sized for any ladder of the handle, so that a second call allocates nothing
    const size_t nr = (size_t)M.ncs * M.nchain;
    if (!M.tscale) {
      double *b;
      if ((rc = mc_alloc(mc, (size_t)M.nchain, &b)) || (rc = mc_alloc(mc, nr, &M.tscale)) || (rc = mc_alloc(mc, nr, &M.tacc_win)) ||
          (rc = mc_alloc(mc, nr, &M.swap_try)) || (rc = mc_alloc(mc, nr, &M.swap_acc)))
        return rc;
      M.beta = b;
    }
    const std::vector<float> s0(nr, mc->step0);
    DZ_HIP(hipMemcpyAsync((void *)M.beta, beta.data(), beta.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    DZ_HIP(hipMemcpyAsync(M.tscale, s0.data(), nr * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    DZ_HIP(hipMemsetAsync(M.tacc_win, 0, nr * sizeof(int), ctx->stream));
    DZ_HIP(hipMemsetAsync(M.swap_try, 0, nr * sizeof(long long), ctx->stream));
    DZ_HIP(hipMemsetAsync(M.swap_acc, 0, nr * sizeof(long long), ctx->stream));
    DZ_HIP(hipStreamSynchronize(ctx->stream));
  }
  M.ntemp = ntemp;
  M.nswap = nswap;
  mc->tmax = tmax;
  mc->beta = beta;
  return 0;
}

int dazim_mc_temper_state(dazim_ctx *ctx, dazim_mc *mc, int *ntemp, float *tmax, int *nswap, double *beta, float *scale,
                          int64_t *swap_try, int64_t *swap_acc) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_temper_state"))) return rc;
  const McDev &M = mc->d;
  if (ntemp) *ntemp = M.ntemp;
  if (tmax) *tmax = mc->tmax;
  if (nswap) *nswap = M.nswap;
  if (M.ntemp == 1) {
    if (beta || scale || swap_try || swap_acc)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_temper_state: the handle is not tempered and keeps no ladder");
    return 0;
  }
  DZ_HIP(hipSetDevice(ctx->device));
  const size_t np = (size_t)M.ncs * (M.ntemp - 1);
  DZ_HIP(mc_get(ctx, beta, M.beta, (size_t)M.ntemp * 8));
  DZ_HIP(mc_get(ctx, scale, M.tscale, (size_t)M.ncs * M.ntemp * 4));
  DZ_HIP(mc_get(ctx, swap_try, M.swap_try, np * 8));
  DZ_HIP(mc_get(ctx, swap_acc, M.swap_acc, np * 8));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// the noise mode of a handle that has not stepped: G = 0 off, else G groups with the validated priors (a0[g], b0[g]) and the group
// grp[p] of every period (null: group 0).  The arrays are sized for MC_MAXGRP groups at the first call, so that a later one allocates
// nothing but chi2g, which one group does not need
static int mc_noise_setup(dazim_ctx *ctx, dazim_mc *mc, int G, const int *grp, const float *a0, const float *b0) {
  McDev &M = mc->d;
  int rc;
  if (G == 0) {
    M.ngrp = 0;
    for (int g = 0; g < MC_MAXGRP; g++) M.ga0[g] = M.gb0[g] = 0.0f;
    return 0;
  }
  DZ_HIP(hipSetDevice(ctx->device));
  const size_t nc = (size_t)M.ncol;
  if (!M.nsum) {
    double *g;
    int *q;
    if ((rc = mc_alloc(mc, 2 * MC_MAXGRP * nc, &M.nsum)) || (rc = mc_alloc(mc, nc, &M.ncnt)) ||
        (rc = mc_alloc(mc, (size_t)MC_MAXGRP * (MC_MAXPER + 1), &g)) || (rc = mc_alloc(mc, (size_t)M.kmax, &q)))
      return rc;
    M.ngam = g;
    M.grp = q;
  }
  if (G > 1 && !M.chi2g && (rc = mc_alloc(mc, MC_MAXGRP * nc, &M.chi2g))) return rc;
  // g(a) = Gamma(a - 1/2) / Gamma(a) at a = a0 + nd / 2 for every nd a cell can have: one table, so that host and device agree
  std::vector<double> gam((size_t)G * (MC_MAXPER + 1));
  for (int g = 0; g < G; g++)
    for (int nd = 0; nd <= MC_MAXPER; nd++) {
      const double a = (double)a0[g] + 0.5 * nd;
      gam[(size_t)g * (MC_MAXPER + 1) + nd] = std::exp(std::lgamma(a - 0.5) - std::lgamma(a));
    }
  std::vector<int> gp((size_t)M.kmax, 0);
  if (grp) gp.assign(grp, grp + M.kmax);
  DZ_HIP(hipMemcpyAsync((void *)M.ngam, gam.data(), gam.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync((void *)M.grp, gp.data(), gp.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemsetAsync(M.nsum, 0, (2 * MC_MAXGRP * nc ? 2 * MC_MAXGRP * nc : 1) * sizeof(double), ctx->stream));
  DZ_HIP(hipMemsetAsync(M.ncnt, 0, (nc ? nc : 1) * sizeof(long long), ctx->stream));
  const std::vector<double> inf(G > 1 ? (size_t)G * nc : 0, (double)INFINITY);
  if (!inf.empty()) DZ_HIP(hipMemcpyAsync(M.chi2g, inf.data(), inf.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  for (int g = 0; g < MC_MAXGRP; g++) {
    M.ga0[g] = g < G ? a0[g] : 0.0f;
    M.gb0[g] = g < G ? b0[g] : 0.0f;
  }
  M.ngrp = G;
  return 0;
}

int dazim_mc_set_noise(dazim_ctx *ctx, dazim_mc *mc, float a0, float b0) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_set_noise"))) return rc;
  if (!(std::isfinite(a0) && a0 >= 0.0f)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise: a0 %g is not finite and >= 0", a0);
  if (a0 > 0.0f && !(std::isfinite(b0) && b0 > 0.0f))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise: b0 %g is not finite and > 0", b0);
  if (mc->nstep > 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise: the handle has done %lld steps", (long long)mc->nstep);
  return mc_noise_setup(ctx, mc, a0 == 0.0f ? 0 : 1, nullptr, &a0, &b0);
}

int dazim_mc_set_noise_groups(dazim_ctx *ctx, dazim_mc *mc, int ngroup, const int *group_of_period, const float *a0, const float *b0) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_set_noise_groups"))) return rc;
  if (!group_of_period || !a0 || !b0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_set_noise_groups");
  if (dz_is_device_ptr(group_of_period) || dz_is_device_ptr(a0) || dz_is_device_ptr(b0))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise_groups: group_of_period, a0 and b0 are host arrays");
  if (ngroup < 1 || ngroup > MC_MAXGRP)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise_groups: ngroup %d outside 1..%d", ngroup, MC_MAXGRP);
  for (int p = 0; p < mc->d.kmax; p++)
    if (group_of_period[p] < 0 || group_of_period[p] >= ngroup)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise_groups: period %d is in group %d of %d", p, group_of_period[p], ngroup);
  int npos = 0;
  for (int g = 0; g < ngroup; g++) {
    if (!(std::isfinite(a0[g]) && a0[g] >= 0.0f))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise_groups: a0 %g of group %d is not finite and >= 0", a0[g], g);
    npos += a0[g] > 0.0f;
  }
  if (npos != 0 && npos != ngroup)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise_groups: a0 is 0 for %d of the %d groups: all of them or none", ngroup - npos,
                   ngroup);
  for (int g = 0; g < ngroup && npos; g++)
    if (!(std::isfinite(b0[g]) && b0[g] > 0.0f))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise_groups: b0 %g of group %d is not finite and > 0", b0[g], g);
  if (mc->nstep > 0)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_noise_groups: the handle has done %lld steps", (long long)mc->nstep);
  return mc_noise_setup(ctx, mc, npos ? ngroup : 0, ngroup > 1 ? group_of_period : nullptr, a0, b0);
}

int dazim_mc_noise_groups_state(dazim_ctx *ctx, dazim_mc *mc, int *ngroup, int *group_of_period, float *a0, float *b0, double *chi2g,
                                double *nsum, int64_t *ncnt) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_noise_groups_state"))) return rc;
  const McDev &M = mc->d;
  if (ngroup) *ngroup = M.ngrp;
  if (!M.ngrp) {
    if (group_of_period || a0 || b0 || chi2g || nsum || ncnt)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_noise_groups_state: no noise scale is switched on");
    return 0;
  }
  if (dz_is_device_ptr(a0) || dz_is_device_ptr(b0))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_noise_groups_state: a0 and b0 are host arrays");
  for (int g = 0; g < M.ngrp; g++) {
    if (a0) a0[g] = M.ga0[g];
    if (b0) b0[g] = M.gb0[g];
  }
  DZ_HIP(hipSetDevice(ctx->device));
  DZ_HIP(mc_get(ctx, group_of_period, M.grp, (size_t)M.kmax * 4));
  DZ_HIP(mc_get(ctx, chi2g, M.ngrp > 1 ? M.chi2g : M.chi2, (size_t)M.ngrp * M.ncol * 8));   // (one group's chi^2_g is chi^2)
  DZ_HIP(mc_get(ctx, nsum, M.nsum, (size_t)2 * M.ngrp * M.ncol * 8));
  DZ_HIP(mc_get(ctx, ncnt, M.ncnt, (size_t)M.ncol * 8));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// dazim_mc_noise_result (single: exactly one group is on) and dazim_mc_noise_groups_result
static int mc_noise_result(dazim_ctx *ctx, dazim_mc *mc, const char *what, bool single, float *lam_mean_u, float *lam_std_u, int *ndata_u) {
  int rc;
  if ((rc = mc_check(ctx, mc, what))) return rc;
  if (!lam_mean_u || !lam_std_u || !ndata_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to %s", what);
  if (single && mc->d.ngrp != 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: dazim_mc_set_noise has not switched the noise scale on", what);
  if (!mc->d.ngrp) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: no noise scale is switched on", what);
  if (mc->d.ncs > 0 && mc->nrec < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: no recorded step yet", what);
  DZ_HIP(hipSetDevice(ctx->device));
  const McDev &M = mc->d;
  const size_t n = (size_t)M.ngrp * M.ncell;
  DzBuf<float> lm, ls;
  DzBuf<int> nd;
  if ((rc = lm.init(ctx, lam_mean_u, n, false, true)) || (rc = ls.init(ctx, lam_std_u, n, false, true)) ||
      (rc = nd.init(ctx, ndata_u, n, false, true)))
    return rc;
  hipLaunchKernelGGL(k_mc_noise_final, dim3((unsigned)((n + MC_WAVE - 1) / MC_WAVE)), dim3(MC_WAVE), 0, ctx->stream, M, lm.dev, ls.dev,
                     nd.dev);
  DZ_HIP(hipGetLastError());
  if ((rc = lm.finish()) || (rc = ls.finish()) || (rc = nd.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int dazim_mc_noise_groups_result(dazim_ctx *ctx, dazim_mc *mc, float *lam_mean_u, float *lam_std_u, int *ndata_u) {
  return mc_noise_result(ctx, mc, "dazim_mc_noise_groups_result", false, lam_mean_u, lam_std_u, ndata_u);
}

int dazim_mc_set_segments(dazim_ctx *ctx, dazim_mc *mc, int nseg, const int *seg_iwave, const int *seg_igr, const int *seg_kmax) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_set_segments"))) return rc;
  if (!seg_iwave || !seg_igr || !seg_kmax) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_set_segments");
  if (dz_is_device_ptr(seg_iwave) || dz_is_device_ptr(seg_igr) || dz_is_device_ptr(seg_kmax))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_segments: seg_iwave, seg_igr and seg_kmax are host arrays");
  if (nseg < 1 || nseg > MC_MAXSEG) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_segments: nseg %d outside 1..%d", nseg, MC_MAXSEG);
  int K = 0;
  for (int s = 0; s < nseg; s++) {
    if (seg_iwave[s] != 1 && seg_iwave[s] != 2)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_segments: segment %d: iwave %d is neither 1 (Love) nor 2 (Rayleigh)", s, seg_iwave[s]);
    if (seg_igr[s] != 0 && seg_igr[s] != 1)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_segments: segment %d: igr %d is neither 0 (phase) nor 1 (group)", s, seg_igr[s]);
    if (seg_kmax[s] < 1 || seg_kmax[s] > MC_MAXPER)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_segments: segment %d: %d periods outside 1..%d", s, seg_kmax[s], MC_MAXPER);
    for (int q = 0; q < s; q++)
      if (seg_iwave[q] == seg_iwave[s] && seg_igr[q] == seg_igr[s])
        return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_segments: segments %d and %d are the same wave type", q, s);
    K += seg_kmax[s];
  }
  if (K != mc->d.kmax)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_segments: the segments hold %d periods, the handle %d", K, mc->d.kmax);
  if (mc->nstep > 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_segments: the handle has done %lld steps", (long long)mc->nstep);
  const bool typed = !(nseg == 1 && seg_iwave[0] == 2 && seg_igr[0] == 0);
  if (typed && mc->nthin > 0)
    return dz_fail(ctx, DAZIM_E_BAD_ARG,
                   "dazim_mc_set_segments: the handle samples Gc/Gs (dazim_mc_set_aniso), whose kernel Lsen_Gsc is Rayleigh-phase: "
                   "other segments than Rayleigh phase alone are refused");
  if (mc->d.nrad > 0) {   // a radial handle keeps Rayleigh before Love, both present
    int nr = 0;
    while (nr < nseg && seg_iwave[nr] == 2) nr++;
    bool ok = nr > 0 && nr < nseg;
    for (int s = nr; s < nseg; s++) ok = ok && seg_iwave[s] == 1;
    if (!ok)
      return dz_fail(ctx, DAZIM_E_BAD_ARG,
                     "dazim_mc_set_segments: the handle is radial (dazim_mc_set_radial): at least one Rayleigh and one Love segment, "
                     "every Rayleigh segment before every Love segment");
    mc->rad_nr = nr;
    mc->rad_kr = 0;
    for (int s = 0; s < nr; s++) mc->rad_kr += seg_kmax[s];
  }
  mc->nseg = nseg;
  for (int s = 0; s < MC_MAXSEG; s++) {
    mc->seg_iwave[s] = s < nseg ? seg_iwave[s] : 0;
    mc->seg_igr[s] = s < nseg ? seg_igr[s] : 0;
    mc->seg_kmax[s] = s < nseg ? seg_kmax[s] : 0;
  }
  mc->typed = typed;
  return 0;
}

int dazim_mc_noise_state(dazim_ctx *ctx, dazim_mc *mc, float *a0, float *b0, double *nsum, int64_t *ncnt) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_noise_state"))) return rc;
  const McDev &M = mc->d;
  if (a0) *a0 = M.ngrp == 1 ? M.ga0[0] : 0.0f;
  if (b0) *b0 = M.ngrp == 1 ? M.gb0[0] : 0.0f;
  if (M.ngrp != 1) {   // (with several groups a0 = b0 = 0 here: the record is dazim_mc_noise_groups_state's)
    if (nsum || ncnt) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_noise_state: dazim_mc_set_noise has not switched the noise scale on");
    return 0;
  }
  DZ_HIP(hipSetDevice(ctx->device));
  DZ_HIP(mc_get(ctx, nsum, M.nsum, (size_t)2 * M.ncol * 8));
  DZ_HIP(mc_get(ctx, ncnt, M.ncnt, (size_t)M.ncol * 8));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int dazim_mc_noise_result(dazim_ctx *ctx, dazim_mc *mc, float *lam_mean_u, float *lam_std_u, int *ndata_u) {
  return mc_noise_result(ctx, mc, "dazim_mc_noise_result", true, lam_mean_u, lam_std_u, ndata_u);
}

int dazim_mc_set_prior(dazim_ctx *ctx, dazim_mc *mc, float smooth, float damp, const float *vref_u) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_set_prior"))) return rc;
  if (!(std::isfinite(smooth) && smooth >= 0.0f) || !(std::isfinite(damp) && damp >= 0.0f))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_prior: smooth %g or damp %g is not finite and >= 0", smooth, damp);
  if (mc->nstep > 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_prior: the handle has done %lld steps", (long long)mc->nstep);
  McDev &M = mc->d;
  if (smooth == 0.0f && damp == 0.0f) {   // (a radial handle with a coupling keeps its prior: vref stays what it was)
    mc->psmooth = mc->pdamp = 0.0f;
    M.ps2 = M.pd2 = 0.0;
    return mc_prior_refresh(ctx, mc, nullptr);
  }
  DZ_HIP(hipSetDevice(ctx->device));
  const size_t nk = (size_t)M.nlay * M.ncell;
  std::vector<float> vref;
  if (vref_u) {
    if ((rc = mc_to_host(ctx, vref_u, nk, vref))) return rc;
    for (size_t e = 0; e < nk; e++)
      if (!std::isfinite(vref[e]))
        return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_set_prior: a non-finite vref at knot %d, cell %d", (int)(e / M.ncell),
                       (int)(e % M.ncell));
  } else if ((rc = mc_vel0_knots(ctx, mc, vref))) {
    return rc;
  }
  M.ps2 = (double)smooth * (double)smooth;
  M.pd2 = (double)damp * (double)damp;
  mc->psmooth = smooth;
  mc->pdamp = damp;
  return mc_prior_refresh(ctx, mc, &vref);
}

int dazim_mc_prior_state(dazim_ctx *ctx, dazim_mc *mc, float *smooth, float *damp, float *vref, double *q) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_prior_state"))) return rc;
  const McDev &M = mc->d;
  if (smooth) *smooth = mc->psmooth;
  if (damp) *damp = mc->pdamp;
  if (!mc->prior) {
    if (vref || q) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_prior_state: dazim_mc_set_prior has not switched the prior on");
    return 0;
  }
  DZ_HIP(hipSetDevice(ctx->device));
  DZ_HIP(mc_get(ctx, vref, M.pref, (size_t)M.nlay * M.ncell * 4));
  DZ_HIP(mc_get(ctx, q, M.pq, (size_t)M.ncol * 8));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int dazim_mc_step(dazim_ctx *ctx, dazim_mc *mc, int kmax, int64_t ncol, const double *pv_u, int record) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_step"))) return rc;
  if (kmax != mc->d.kmax || ncol != mc->d.ncol)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_step: curves [%d][%lld] for a handle of [%d][%ld]", kmax, (long long)ncol,
                   mc->d.kmax, mc->d.ncol);
  if ((!pv_u && ncol > 0) || (record != 0 && record != 1)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_step");
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_join_aux(ctx))) return rc;
  DzBuf<double> pv;
  if ((rc = pv.init(ctx, pv_u, (size_t)kmax * ncol, true, false))) return rc;
  if ((rc = mc_launch_step(ctx, mc, pv.dev, record))) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  float ms = 0.0f;
  if (mc->d.ncs > 0) DZ_HIP(hipEventElapsedTime(&ms, mc->e0, mc->e1));
  ctx->ksec["mc_step"] = ms * 1e-3;
  return 0;
}

int dazim_mc_run(dazim_ctx *ctx, dazim_mc *mc, const float *depz, float sublayers, const double *periods, int nburn, int nsample,
                 int64_t *n_no_root) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_run"))) return rc;
  if (!depz || !periods || nburn < 0 || nsample < 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_run");
  if (dz_is_device_ptr(depz) || dz_is_device_ptr(periods))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_run: depz and periods are host arrays");
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_join_aux(ctx))) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  unsigned long long c0[2] = {0, 0}, c1[2] = {0, 0};
  DZ_HIP(hipMemcpy(c0, mc->d.counters, 16, hipMemcpyDeviceToHost));
  double t_disp = 0.0, t_step = 0.0, t_aniso = 0.0;
  int64_t dec0 = mc->nrec_dec, passes = 0, skip0 = 0;
  if (mc->nthin > 0) {
    skip0 = mc_aniso_skipped(ctx, mc, &rc);
    if (rc) return rc;
  }
  const int nstep = nburn + nsample;
  bool has_rc = false;   // a Rayleigh-phase segment among the typed ones: both dispersion timers run
  for (int q = 0; q < mc->nseg; q++) has_rc = has_rc || (mc->seg_iwave[q] == 2 && mc->seg_igr[q] == 0);
  for (int s = 0; s < nstep && mc->d.ncs > 0; s++) {
    int nf = 0;
    // curves only, one column per chain: nx = ncol, ny = 1 (the call ends with a wait for the stream: the step enqueued before it
    // has finished when it returns)
    if (mc->d.nrad > 0) {   // the Rayleigh segments on the Vsv model, the Love segments on the Vsh model (rows n..2n of prop)
      const int n = mc->d.nrad, nr = mc->rad_nr, kr = mc->rad_kr;
      int nfh = 0;
      if ((rc = dazim_dispersion_kernels_typed(ctx, (int)mc->d.ncol, 1, n + 1, mc->d.vsv, depz, sublayers, nr, mc->seg_iwave, mc->seg_igr,
                                               mc->seg_kmax, periods, mc->pv, nullptr, nullptr, nullptr, &nf)))
        return rc;
      t_disp += (nr > 1 || !has_rc ? ctx->ksec["disp_typed"] : 0.0) + (has_rc ? ctx->ksec["disp"] : 0.0);
      if ((rc = dazim_dispersion_kernels_typed(ctx, (int)mc->d.ncol, 1, n + 1, mc->d.prop + (size_t)n * mc->d.ncol, depz, sublayers,
                                               mc->nseg - nr, mc->seg_iwave + nr, mc->seg_igr + nr, mc->seg_kmax + nr, periods + kr,
                                               mc->pv + (size_t)kr * mc->d.ncol, nullptr, nullptr, nullptr, &nfh)))
        return rc;
      t_disp += ctx->ksec["disp_typed"];
      nf += nfh;
    } else if (mc->typed) {   // (every segment's curves; a Rayleigh-phase segment goes through the call below inside it)
      if ((rc = dazim_dispersion_kernels_typed(ctx, (int)mc->d.ncol, 1, mc->d.nz, mc->d.prop, depz, sublayers, mc->nseg, mc->seg_iwave,
                                               mc->seg_igr, mc->seg_kmax, periods, mc->pv, nullptr, nullptr, nullptr, &nf)))
        return rc;
      t_disp += ctx->ksec["disp_typed"] + (has_rc ? ctx->ksec["disp"] : 0.0);
    } else {
      if ((rc = dazim_dispersion_kernels(ctx, (int)mc->d.ncol, 1, mc->d.nz, mc->d.prop, depz, sublayers, mc->d.kmax, periods, mc->pv,
                                         nullptr, nullptr, nullptr, &nf)))
        return rc;
      t_disp += ctx->ksec["disp"];
    }
    if (s > 0) {
      float ms = 0.0f;
      DZ_HIP(hipEventElapsedTime(&ms, mc->e0, mc->e1));
      t_step += ms * 1e-3;
    }
    if ((rc = mc_launch_step(ctx, mc, mc->pv, s >= nburn ? 1 : 0))) return rc;
    if (mc->nthin > 0 && s >= nburn && mc->nrec % mc->nthin == 0) {   // a Gc/Gs pass: it reads the chains, writes its own arrays
      const auto ta = std::chrono::steady_clock::now();
      if ((rc = mc_aniso_pass(ctx, mc, depz, sublayers, periods))) return rc;
      t_aniso += std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
      passes++;
    }
  }
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (nstep > 0 && mc->d.ncs > 0) {
    float ms = 0.0f;
    DZ_HIP(hipEventElapsedTime(&ms, mc->e0, mc->e1));
    t_step += ms * 1e-3;
  }
  int64_t skip1 = 0;
  if (mc->nthin > 0) {
    skip1 = mc_aniso_skipped(ctx, mc, &rc);
    if (rc) return rc;
  }
  DZ_HIP(hipMemcpy(c1, mc->d.counters, 16, hipMemcpyDeviceToHost));
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const double dec = (double)(mc->nrec_dec - dec0) * (double)(mc->d.ncol / mc->d.ntemp);   // the recorded (rung-0) chains'
  ctx->ksec["mc"] = wall;
  ctx->ksec["mc.disp"] = t_disp;
  ctx->ksec["mc.step"] = t_step;
  ctx->ksec["mc.steps"] = mc->d.ncs > 0 ? nstep : 0;
  ctx->ksec["mc.accept"] = dec > 0 ? (double)(c1[1] - c0[1]) / dec : 0.0;
  ctx->ksec["mc.no_root"] = (double)(c1[0] - c0[0]);
  ctx->ksec["mc.aniso"] = t_aniso;
  ctx->ksec["mc.aniso_passes"] = (double)passes;
  ctx->ksec["mc.aniso_skipped"] = (double)(skip1 - skip0);
  int cov_cells = 0;
  if (mc->kind == 1 && mc->d.ncs > 0) {
    std::vector<int> set((size_t)mc->d.ncs);
    DZ_HIP(hipMemcpy(set.data(), mc->d.cov_set, set.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int v : set) cov_cells += v;
  }
  // the swap acceptance of every (cell, rung pair), over all the handle's steps
  double swap_min = 0.0, swap_med = 0.0;
  if (mc->d.ntemp > 1 && mc->d.ncs > 0) {
    const size_t np = (size_t)mc->d.ncs * (mc->d.ntemp - 1);
    std::vector<long long> tr(np), ac(np);
    DZ_HIP(hipMemcpy(tr.data(), mc->d.swap_try, np * sizeof(long long), hipMemcpyDeviceToHost));
    DZ_HIP(hipMemcpy(ac.data(), mc->d.swap_acc, np * sizeof(long long), hipMemcpyDeviceToHost));
    std::vector<double> rate;
    for (size_t e = 0; e < np; e++)
      if (tr[e] > 0) rate.push_back((double)ac[e] / (double)tr[e]);
    if (!rate.empty()) {
      std::sort(rate.begin(), rate.end());
      swap_min = rate.front();
      swap_med = 0.5 * (rate[(rate.size() - 1) / 2] + rate[rate.size() / 2]);
    }
  }
  ctx->ksec["mc.ntemp"] = mc->d.ntemp;
  ctx->ksec["mc.swap_min"] = swap_min;
  ctx->ksec["mc.swap_med"] = swap_med;
  ctx->ksec["mc.proposal"] = mc->kind;
  ctx->ksec["mc.noise"] = std::min(mc->d.ngrp, 2);
  ctx->ksec["mc.noise_groups"] = mc->d.ngrp;
  ctx->ksec["mc.prior"] = mc->prior;
  ctx->ksec["mc.radial"] = mc->d.nrad > 0;
  ctx->ksec["mc.cov_cells"] = cov_cells;
  if (n_no_root) *n_no_root = (int64_t)(c1[0] - c0[0]);
  return 0;
}

int dazim_mc_state(dazim_ctx *ctx, dazim_mc *mc, float *cur, double *chi2, float *scale, int64_t *step, double *sums, unsigned *hist,
                   int64_t *accepted, float *best, double *best_chi2) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_state"))) return rc;
  DZ_HIP(hipSetDevice(ctx->device));
  const McDev &M = mc->d;
  DZ_HIP(mc_get(ctx, cur, M.cur, (size_t)M.nz * M.ncol * 4));
  DZ_HIP(mc_get(ctx, chi2, M.chi2, (size_t)M.ncol * 8));
  DZ_HIP(mc_get(ctx, scale, M.scale, (size_t)M.ncs * 4));
  DZ_HIP(mc_get(ctx, sums, M.sums, (size_t)2 * M.nlay * M.ncol * 8));
  DZ_HIP(mc_get(ctx, hist, M.hist, (size_t)M.ncs * M.nlay * M.nbin * 4));
  DZ_HIP(mc_get(ctx, accepted, M.accepted, (size_t)M.ncol * 8));
  DZ_HIP(mc_get(ctx, best, M.best, (size_t)M.nlay * M.ncs * 4));
  DZ_HIP(mc_get(ctx, best_chi2, M.best_chi2, (size_t)M.ncs * 8));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (step) *step = mc->nstep;
  return 0;
}

int dazim_mc_result(dazim_ctx *ctx, dazim_mc *mc, float *mean_u, float *std_u, float *q_u, float *best_u, float *rhat_u, float *accept_u,
                    float *chi2_u) {
  int rc;
  if ((rc = mc_check(ctx, mc, "dazim_mc_result"))) return rc;
  if (!mean_u || !std_u || !q_u || !best_u || !rhat_u || !accept_u || !chi2_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_mc_result");
  if (mc->d.ncs > 0 && mc->nrec < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_mc_result: no recorded step yet");
  DZ_HIP(hipSetDevice(ctx->device));
  const McDev &M = mc->d;
  const size_t nk = (size_t)M.nlay * M.ncell;
  DzBuf<float> mean, stdv, q, best, rhat, acc, chi2;
  if ((rc = mean.init(ctx, mean_u, nk, false, true)) || (rc = stdv.init(ctx, std_u, nk, false, true)) ||
      (rc = q.init(ctx, q_u, 3 * nk, false, true)) || (rc = best.init(ctx, best_u, nk, false, true)) ||
      (rc = rhat.init(ctx, rhat_u, nk, false, true)) || (rc = acc.init(ctx, accept_u, (size_t)M.ncell, false, true)) ||
      (rc = chi2.init(ctx, chi2_u, (size_t)M.ncell, false, true)))
    return rc;
  hipLaunchKernelGGL(k_mc_final, dim3((unsigned)M.ncell), dim3(MC_WAVE), 0, ctx->stream, M, (long long)mc->nrec, (long long)mc->nrec_dec,
                     mean.dev, stdv.dev, q.dev, best.dev, rhat.dev, acc.dev, chi2.dev);
  DZ_HIP(hipGetLastError());
  if ((rc = mean.finish()) || (rc = stdv.finish()) || (rc = q.finish()) || (rc = best.finish()) || (rc = rhat.finish()) ||
      (rc = acc.finish()) || (rc = chi2.finish()))
    return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int dazim_mc_free(dazim_ctx *ctx, dazim_mc *mc) {
  if (!mc) return 0;
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  return mc_release(mc);
}

}  // extern "C"
