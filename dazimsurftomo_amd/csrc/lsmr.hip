// lsmr.hip -- K7 of SURVEY.md: the fp32 LSMR solver (inv/lsmrModule.f90:36) on the two products of sparse.hip.  Vectors and
// scalar recurrences live on the device; the host (LsmrSolve below) only enqueues kernels, one stage of the algorithm per function.
#include "sparse_internal.h"

#include <rccl/rccl.h>
#include <cstdlib>

namespace {

// ---- small vector kernels (all O(m+n), negligible next to the products) ----------------------
// res[0] = sqrt(sum part[0..np)) as fp32 (the reference's dnrm2 result type), res[1] = the sum
__global__ void finish_norm(const double *part, int np, float *res, double *res_d) {
  double t = 0.0;
  for (int i = threadIdx.x; i < np; i += 64) t += part[i];
  t = wave_sum(t);
  if (threadIdx.x == 0) {
    res[0] = (float)sqrt(t);
    if (res_d) res_d[0] = t;
  }
}
// res[0] = sqrt(*sum) (after the all-reduce of a distributed norm)
__global__ void k_sqrt_sum(const double *sum, float *res) { res[0] = (float)sqrt(sum[0]); }
// v = w + sign*beta*v with the partial of ||v||^2 (distributed A^T u: w is the all-reduced product)
__global__ void k_axpby_norm(int64_t n, const float *w, float *v, const float *beta_p, float beta_sign, double *part,
                             const int *guard) {
  if (guard && *guard) return;
  const float beta = beta_p ? beta_sign * beta_p[0] : beta_sign;
  double sq = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) {
    const float o = beta * v[i] + w[i];
    v[i] = o;
    sq += (double)o * o;
  }
  block_partial(sq, part);
}
__global__ void k_sumsq(int64_t n, const float *x, double *part) {
  double v = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) v += (double)x[i] * x[i];
  block_partial(v, part);
}
// x *= sign/ (*d)   or  x *= sign * (*d)
__global__ void k_scal_inv(int64_t n, float *x, const float *d, float sign) {
  const float a = sign * (1.0f / d[0]);
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) x[i] = a * x[i];
}
__global__ void k_copy(int64_t n, const float *a, float *b) {
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) b[i] = a[i];
}
// ---- LSMR with the scalar recurrences on the device (inv/lsmrModule.f90:484-616) ----------------------------------------
// The host only enqueues kernels: alpha, beta, the plane rotations, the norm estimates and the stopping tests live in one
// LsmrState in HBM, so an iteration needs no host round trip.  The stop flag is looked at every few iterations; the
// iterations enqueued behind the one that stopped return at once (every kernel of the loop starts with `if (*guard) return`),
// so x, itn and the norm estimates are exactly those of the stopping iteration.
struct LsmrState {
  float alpha, beta, alphabar, zetabar, rho, rhobar, cbar, sbar;
  float betadd, betad, rhodold, tautildeold, thetatilde, zeta, d;
  float normA2, maxrbar, minrbar, normb, ctol;
  float normA, condA, normr, normAr, normx;
  float damp, atol, btol;
  float alpha_new;   // alpha of the running iteration: k_alpha_update -> k_tests
  int itn, istop, itnlim;
  int stop;          // != 0: LSMR has stopped; guard of the first half-step (u = A v - alpha u)
  int stop2;         // stop, or beta == 0 in the running iteration: guard of the second half-step (skipped as a block, :490-503)
};
__device__ __forceinline__ float dz_d2norm(float a, float bb) {   // d2norm, :708-721
  const float scale = fabsf(a) + fabsf(bb);
  if (scale == 0.0f) return 0.0f;
  return scale * sqrtf((a / scale) * (a / scale) + (bb / scale) * (bb / scale));
}
// one pass of the scalar recurrences, statement for statement :506-588 (fp32, no contraction); s -> state after the
// iteration that produced (alpha, beta); f1..f3 are the coefficients of the hbar / x / h updates (:539-541)
__device__ __forceinline__ void lsmr_recur(LsmrState &s, float alpha, float beta, float &f1, float &f2, float &f3) {
  const float damp = s.damp;
  float alphabar = s.alphabar, zetabar = s.zetabar, rho = s.rho, rhobar = s.rhobar, cbar = s.cbar, sbar = s.sbar;
  float betadd = s.betadd, betad = s.betad, rhodold = s.rhodold, tautildeold = s.tautildeold, thetatilde = s.thetatilde;
  float zeta = s.zeta, d = s.d, normA2 = s.normA2, maxrbar = s.maxrbar, minrbar = s.minrbar;
  const int itn = s.itn + 1;
  const float alphahat = dz_d2norm(alphabar, damp);
  const float chat = alphabar / alphahat, shat = damp / alphahat;
  const float rhoold = rho;
  rho = dz_d2norm(alphahat, beta);
  const float c = alphahat / rho, sn = beta / rho;
  const float thetanew = sn * alpha;
  alphabar = c * alpha;
  const float rhobarold = rhobar, zetaold = zeta;
  const float thetabar = sbar * rho, rhotemp = cbar * rho;
  rhobar = dz_d2norm(cbar * rho, thetanew);
  cbar = cbar * rho / rhobar;
  sbar = thetanew / rhobar;
  zeta = cbar * zetabar;
  zetabar = -sbar * zetabar;
  f1 = thetabar * rho / (rhoold * rhobarold);
  f2 = zeta / (rho * rhobar);
  f3 = thetanew / rho;
  const float betaacute = chat * betadd, betacheck = -shat * betadd;
  const float betahat = c * betaacute;
  betadd = -sn * betaacute;
  const float thetatildeold = thetatilde;
  const float rhotildeold = dz_d2norm(rhodold, thetabar);
  const float ctildeold = rhodold / rhotildeold, stildeold = thetabar / rhotildeold;
  thetatilde = stildeold * rhobar;
  rhodold = ctildeold * rhobar;
  betad = -stildeold * betad + ctildeold * betahat;
  tautildeold = (zetaold - thetatildeold * tautildeold) / rhotildeold;
  const float taud = (zeta - thetatilde * tautildeold) / rhodold;
  d = d + betacheck * betacheck;
  s.normr = sqrtf(d + (betad - taud) * (betad - taud) + betadd * betadd);
  normA2 = normA2 + beta * beta;
  s.normA = sqrtf(normA2);
  normA2 = normA2 + alpha * alpha;
  maxrbar = fmaxf(maxrbar, rhobarold);
  if (itn > 1) minrbar = fminf(minrbar, rhobarold);
  s.condA = fmaxf(maxrbar, rhotemp) / fminf(minrbar, rhotemp);
  s.normAr = fabsf(zetabar);
  s.alpha = alpha; s.beta = beta; s.alphabar = alphabar; s.zetabar = zetabar; s.rho = rho; s.rhobar = rhobar; s.cbar = cbar;
  s.sbar = sbar; s.betadd = betadd; s.betad = betad; s.rhodold = rhodold; s.tautildeold = tautildeold;
  s.thetatilde = thetatilde; s.zeta = zeta; s.d = d; s.normA2 = normA2; s.maxrbar = maxrbar; s.minrbar = minrbar;
  s.itn = itn;
}
// sum of np partials by the first wavefront of the block in a fixed order: every block, every launch gets the same bits
__device__ __forceinline__ double block_total(const double *part, int np) {
  __shared__ double s_t;
  if (threadIdx.x < 64) {
    double t = 0.0;
    for (int i = threadIdx.x; i < np; i += 64) t += part[i];
    t = wave_sum(t);
    if (threadIdx.x == 0) s_t = t;
  }
  __syncthreads();
  return s_t;
}
// beta = ||u|| from the partials of the product that wrote u (or from the all-reduced sum); u /= beta; localVEnqueue(v)
// (:487-492).  beta == 0 skips the second half-step of this iteration (stop2).
__global__ void k_beta_scal_u(int64_t m, float *u, const double *part, int np, const double *sum_in, int64_t n, const float *v,
                              float *lv_slot, LsmrState *S) {
  if (S->stop) return;
  const double t = sum_in ? sum_in[0] : block_total(part, np);
  const float beta = (float)sqrt(t);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    S->beta = beta;
    S->stop2 = !(beta > 0.0f);
  }
  if (!(beta > 0.0f)) return;
  const float a = 1.0f / beta;
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < m; i += (int64_t)gridDim.x * VB) u[i] = a * u[i];
  if (lv_slot)
    for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) lv_slot[i] = v[i];
}
// Row-sharded solve, ONE collective per iteration (round 5).  The two all-reduces of an iteration used to depend on each other:
// ||u||^2 had to be summed over the ranks before u could be scaled, and only the scaled u went into A_p^T u_p.  A^T is linear, so
// each rank now scales its shard by its OWN norm (u_p / beta_p: entries <= 1, which the fixed-point scatter relies on), forms
// w_p = beta_p A_p^T (u_p / beta_p) = A_p^T u_p, and ONE collective carries the n floats of w and the double beta_p^2 (round 6: an
// all-gather of the ranks' buffers, summed in rank order by k_beta_axpby; a grouped ncclAllReduce with option comm.allreduce);
// afterwards beta = sqrt(sum beta_p^2), v = w / beta - beta v and u_p <- (u_p / beta_p) (beta_p / beta).
// k_local_norm_scal: beta_p^2 -> sum[0], beta_p -> bp[0], u_p /= beta_p.
__global__ void k_local_norm_scal(int64_t m, float *u, const double *part, int np, double *sum, float *bp, const LsmrState *S) {
  if (S->stop) return;
  const double t = block_total(part, np);
  const float b = (float)sqrt(t);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sum[0] = t;
    bp[0] = b;
  }
  if (!(b > 0.0f)) return;
  const float a = 1.0f / b;
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < m; i += (int64_t)gridDim.x * VB) u[i] = a * u[i];
}
__global__ void k_scale_by(int64_t n, float *w, const float *f, const int *guard) {
  if (guard && *guard) return;
  const float a = f[0];
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) w[i] = a * w[i];
}
// after the collective: beta (:487), localVEnqueue(v) (:490-492), u_p = u / beta, v = A^T u - beta v (:496-497) from w = sum_p A_p^T u_p,
// partials of ||v||^2.  beta == 0 skips the second half-step (stop2), as in k_beta_scal_u.  The collective is an all-gather: rank r's
// n floats of w_r and its double beta_r^2 (at byte offset sum_off) sit at gathered + r*stride, and the sums over the ranks are formed
// HERE, in rank order -- the same bits on every rank and with every transport (SURVEY 8e "fix reduction order").  nr = 1: `gathered`
// holds sums already (option comm.allreduce).
__global__ void k_beta_axpby(int64_t m, float *u, int64_t n, float *v, const char *__restrict__ gathered, int nr, size_t stride,
                             size_t sum_off, const float *bp, float *lv_slot, double *part, LsmrState *S) {
  if (S->stop) return;
  double t = *reinterpret_cast<const double *>(gathered + sum_off);
  for (int r = 1; r < nr; r++) t += *reinterpret_cast<const double *>(gathered + (size_t)r * stride + sum_off);
  const float beta = (float)sqrt(t);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    S->beta = beta;
    S->stop2 = !(beta > 0.0f);
  }
  double sq = 0.0;
  if (beta > 0.0f) {
    const float rb = 1.0f / beta, ru = bp[0] * rb;
    for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < m; i += (int64_t)gridDim.x * VB) u[i] = ru * u[i];
    for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) {
      const float vi = v[i];
      if (lv_slot) lv_slot[i] = vi;
      float w = reinterpret_cast<const float *>(gathered)[i];
      for (int r = 1; r < nr; r++) w += reinterpret_cast<const float *>(gathered + (size_t)r * stride)[i];
      const float o = -beta * vi + rb * w;
      v[i] = o;
      sq += (double)o * o;
    }
  }
  block_partial(sq, part);
}
// local reorthogonalisation step q (localVOrtho, inv/lsmrModule.f90:733-748), modified Gram-Schmidt:
// d = sum(part_in) (the dot of v with lv_prev computed by the previous launch); v -= d*lv_prev;
// part_out = partial dots of the updated v with lv_next, or -- last step, lv_next null -- partials of ||v||^2.
__global__ void k_reorth(int64_t n, float *v, const float *lv_prev, const double *part_in, int np,
                         const float *lv_next, double *part_out, const int *guard) {
  if (guard && *guard) return;
  __shared__ float s_d;
  if (lv_prev) {
    if (threadIdx.x < 64) {
      double t = 0.0;
      for (int i = threadIdx.x; i < np; i += 64) t += part_in[i];
      t = wave_sum(t);
      if (threadIdx.x == 0) s_d = (float)t;
    }
    __syncthreads();
  }
  const float d = lv_prev ? s_d : 0.0f;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) {
    float vi = v[i];
    if (lv_prev) {
      vi = vi - d * lv_prev[i];
      v[i] = vi;
    }
    acc += lv_next ? (double)vi * lv_next[i] : (double)vi * vi;
  }
  if (part_out) block_partial(acc, part_out);
}
// The same chain in ONE launch (round 5; the chain above is lim + 1 launches of ~5 us each on an n-float vector -- 54 of the 255 us
// of a test4_Yunnan iteration).  At most RC_BLOCKS workgroups of 1024 threads hold v in registers (E elements per thread) and walk
// the window in the reference's order -- d = v . lv_q, v -= d lv_q, modified Gram-Schmidt: each dot sees the subtractions before it
// -- with a grid barrier between a step's partial dots and its subtraction.  The sums are taken in a fixed order (per block, then
// over the blocks by every block alike), so the result does not depend on arrival order; it differs from the chain's only in the
// grouping of the partial sums.  (Taking all dots of the window at once -- classical Gram-Schmidt, two launches -- was tried first:
// the iterates leave the reference's within eight iterations, 1.2e-2 relative on the test system of tests/test_sparse_gpu.py.)
// The barrier: one counter per solve, never reset, target = (barriers so far) x blocks; release / acquire at agent scope
// (MI355X_MICROARCH.md, inter-workgroup visibility).  All blocks must be resident at once: the host launches at most as many as the
// occupancy query allows on the device and takes the chain below otherwise (or on a CU-masked stream).
constexpr int RC_BLOCKS = 64, RC_THREADS = 1024, RC_EMAX = 16;
template <int E>
__global__ __launch_bounds__(RC_THREADS) void k_reorth_coop(int64_t n, float *__restrict__ v, const float *__restrict__ lv, int lim,
                                                             double *__restrict__ part2, double *__restrict__ part_out,
                                                             unsigned *bar, unsigned bar_base, const int *guard) {
  const int G = gridDim.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (guard && *guard) {   // skipped half-step: the counter still advances by what the host has booked for this launch
    if (tid == 0 && G > 1) __hip_atomic_fetch_add(bar, (unsigned)lim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  __shared__ double s_w[RC_THREADS / 64];
  __shared__ float s_d;
  float vr[E];
  int64_t idx[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    idx[e] = (int64_t)blockIdx.x * RC_THREADS + tid + (int64_t)e * G * RC_THREADS;
    vr[e] = idx[e] < n ? v[idx[e]] : 0.0f;
  }
  for (int q = 0; q < lim; q++) {
    float lr[E];
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      lr[e] = idx[e] < n ? lv[(size_t)q * n + idx[e]] : 0.0f;
      acc += (double)vr[e] * lr[e];
    }
    acc = wave_sum(acc);
    if (lane == 0) s_w[w] = acc;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int i = 0; i < RC_THREADS / 64; i++) t += s_w[i];
      part2[(size_t)(q & 1) * RC_BLOCKS + blockIdx.x] = t;
      if (G > 1) {   // (one release fence, relaxed polls, one acquire fence: an acquiring load per poll invalidates caches every time)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned target = bar_base + (unsigned)(q + 1) * (unsigned)G;
        while ((int)(__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
    }
    __syncthreads();
    if (tid < 64) {   // the dot: the blocks' partials in block order, by every block alike
      double t = 0.0;
      for (int i = lane; i < G; i += 64) t += part2[(size_t)(q & 1) * RC_BLOCKS + i];
      t = wave_sum(t);
      if (tid == 0) s_d = (float)t;
    }
    __syncthreads();
    const float d = s_d;
#pragma unroll
    for (int e = 0; e < E; e++) vr[e] = vr[e] - d * lr[e];
  }
  double sq = 0.0;
#pragma unroll
  for (int e = 0; e < E; e++)
    if (idx[e] < n) {
      v[idx[e]] = vr[e];
      sq += (double)vr[e] * vr[e];
    }
  sq = wave_sum(sq);
  __syncthreads();
  if (lane == 0) s_w[w] = sq;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < RC_THREADS / 64; i++) t += s_w[i];
    part_out[blockIdx.x] = t;
  }
}
// alpha = ||v|| (:499); v /= alpha; rotations; hbar = h - f1*hbar ; x += f2*hbar ; h = v - f3*h (:539-541); partials of ||x||^2.
// Every block evaluates the recurrences from the (read-only here) state; k_tests commits them.
__global__ void k_alpha_update(int64_t n, float *v, float *h, float *hbar, float *x, const double *part, int np,
                               double *partx, LsmrState *S) {
  if (S->stop) return;
  __shared__ float s_f[4];
  const bool half2 = !S->stop2;                  // beta > 0: v was renewed and alpha with it (else both keep their values)
  const double t = half2 ? block_total(part, np) : 0.0;
  if (threadIdx.x == 0) {
    LsmrState st = *S;
    const float alpha = half2 ? (float)sqrt(t) : st.alpha;
    float f1, f2, f3;
    lsmr_recur(st, alpha, st.beta, f1, f2, f3);
    s_f[0] = f1; s_f[1] = f2; s_f[2] = f3; s_f[3] = alpha;
    if (blockIdx.x == 0) S->alpha_new = alpha;
  }
  __syncthreads();
  const float f1 = s_f[0], f2 = s_f[1], f3 = s_f[2], alpha = s_f[3];
  const bool scal = half2 && alpha > 0.0f;
  const float a = scal ? 1.0f / alpha : 1.0f;
  double sq = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) {
    float vi = v[i];
    if (scal) {
      vi = a * vi;
      v[i] = vi;
    }
    const float hb = h[i] - f1 * hbar[i];
    const float xn = x[i] + f2 * hb;
    hbar[i] = hb;
    x[i] = xn;
    h[i] = vi - f3 * h[i];
    sq += (double)xn * xn;
  }
  block_partial(sq, partx);
}
// normx (:590), stopping tests (:595-616), commit of the state, one trace record per iteration (the columns of the
// reference's iteration log, format 1500 at :679, plus test3 and rtol which decide whether the line is printed)
__global__ void k_tests(const double *partx, int npx, const float *x, LsmrState *S, dazim_lsmr_rec *trace, int trace_cap) {
  if (S->stop) return;
  const double t = block_total(partx, npx);
  if (threadIdx.x != 0) return;
  LsmrState st = *S;
  float f1, f2, f3;
  lsmr_recur(st, st.alpha_new, st.beta, f1, f2, f3);
  const float normx = (float)sqrt(t);
  st.normx = normx;
  const float test1 = st.normr / st.normb, test2 = st.normAr / (st.normA * st.normr), test3 = 1.0f / st.condA;
  const float t1 = test1 / (1.0f + st.normA * normx / st.normb);
  const float rtol = st.btol + st.atol * st.normA * normx / st.normb;
  int istop = 0;
  if (st.itn >= st.itnlim) istop = 7;
  if (1.0f + test3 <= 1.0f) istop = 6;
  if (1.0f + test2 <= 1.0f) istop = 5;
  if (1.0f + t1 <= 1.0f) istop = 4;
  if (test3 <= st.ctol) istop = 3;
  if (test2 <= st.atol) istop = 2;
  if (test1 <= rtol) istop = 1;
  st.istop = istop;
  st.stop = istop != 0;
  st.stop2 = st.stop;
  if (trace && st.itn < trace_cap) {
    dazim_lsmr_rec r;
    r.itn = st.itn; r.x1 = x[0]; r.normr = st.normr; r.normAr = st.normAr; r.test1 = test1; r.test2 = test2;
    r.test3 = test3; r.rtol = rtol; r.normA = st.normA; r.condA = st.condA;
    trace[st.itn] = r;
  }
  *S = st;
}

constexpr int CHECK = 8, NSLOT = 2;   // iterations per batch; pinned state slots the batches' final states are copied to in turn
struct LsmrArgs {   // the arguments of dazim_lsmr_traced, in its order
  dazim_ctx *ctx; const dazim_csr *A; const float *b_u;
  float damp, atol, btol, conlim; int itnlim, localSize; float *x_u;
  int *istop_o, *itn_o; float *normA_o, *condA_o, *normr_o, *normAr_o, *normx_o;
  dazim_lsmr_rec *trace; int trace_cap, *trace_n;
};
// One solve.  The stages run in the order they are defined in; between agree() and the end any failure goes through leave().
struct LsmrSolve : LsmrArgs {
  const int64_t m, n;
  DzComm *comm;   // non-null: A, b are this rank's rows of one global system
  DzBuf<float> b, x;
  double *d_sum = nullptr;
  long long *d_cons = nullptr;
  float *wbuf = nullptr;   // this rank's n floats of A_p^T u_p | its double beta_p^2 ...
  char *gbuf = nullptr;    // ... of every rank
  const size_t w_sum_off, w_bytes;
  int64_t m_glob;
  int localVecs = 0;
  float *u = nullptr, *v = nullptr, *h = nullptr, *hbar = nullptr, *localV = nullptr, *d_scal = nullptr;
  double *part = nullptr, *part2 = nullptr, *partx = nullptr;
  LsmrState *S = nullptr;
  dazim_lsmr_rec *d_trace = nullptr;
  const int gm, gn, bn, bm;
  int gm_t, gn_t;   // partial counts of the last products
  struct Pinned {   // pinned state copies + events, released on every exit path
    LsmrState *h = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, done[NSLOT] = {}, ta[NSLOT][4] = {};
    ~Pinned() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      for (int i = 0; i < NSLOT; i++) {
        if (done[i]) (void)hipEventDestroy(done[i]);
        for (int j = 0; j < 4; j++)
          if (ta[i][j]) (void)hipEventDestroy(ta[i][j]);
      }
      if (h) (void)hipHostFree(h);
    }
  } guard;
  LsmrState *h_state = nullptr;   // NSLOT batch slots, then the state the host works on
  float *h_scal = nullptr;
  const int *g1 = nullptr, *g2 = nullptr;   // &S->stop, &S->stop2: the guards of the two half-steps
  int istop = 0, itn = 0, ntrace = 0;
  float normA = 0, condA = 0, normr = 0, normAr = 0, normx = 0, normb = 0;
  // max |u| as A^T u's fixed-point scatter form is told it: u is normalised, so 1 -- unless ||b|| is NaN or Inf (b holds one): then
  // u does too, and that value sends every A^T u of the solve to the gather form, which propagates it
  float ymax = 1.0f;
  double t_spmv = 0, t_spmvt = 0;
  int n_spmv = 0, n_spmvt = 0;
  long n_enq = 0;       // iterations enqueued
  long n_coll = 0;      // collectives issued inside the iteration loop (row-sharded solve)
  bool rccl_allreduce = false;
  int host_syncs = 0;   // host waits on the device inside the iteration loop (one per examined batch of CHECK iterations)
  int coop_max = 0, rcb = 0;   // k_reorth_coop: workgroups the device holds at once, workgroups of a launch
  int64_t per_thread = 0;      // ... elements of v per thread
  unsigned reorth_barriers = 0;   // arrivals booked at the grid barrier of k_reorth_coop so far (its counter is zeroed in start(), once)

  explicit LsmrSolve(const LsmrArgs &a)
      : LsmrArgs(a), m(A->m), n(A->n), comm((DzComm *)ctx->comm), w_sum_off((((size_t)n * 4 + 7) / 8) * 8), w_bytes(w_sum_off + 8),
        m_glob(m), gm(dz_spmv_blocks(ctx, m, n)), gn(dz_spmv_blocks(ctx, n, m)), bn(nblk(n, NPART)), bm(nblk(m, NPART)), gm_t(gm),
        gn_t(gn) {}

  // ---- everything that can fail locally comes first, so that a row-sharded solve can agree on it before any rank waits in
  // a collective for a rank that has already returned ----
  int alloc() {
    int r;
    if ((r = b.init(ctx, b_u, m, true, false)) || (r = x.init(ctx, x_u, n, false, true))) return r;
    if (comm) {   // (the consensus words come from the scratch pool too: inside the voted set-up)
      if ((r = dz_scratch(ctx, "lsmr.cons", 8, &d_cons)) || (r = dz_scratch(ctx, "lsmr.sum", 8, &d_sum)) ||
          (r = dz_scratch(ctx, "lsmr.w", w_bytes / 4, &wbuf)) || (r = dz_scratch(ctx, "lsmr.gather", w_bytes * (size_t)comm->nranks, &gbuf)))
        return r;
    }
    const int npart = gm > gn ? (gm > NPART ? gm : NPART) : (gn > NPART ? gn : NPART);
    if ((r = dz_scratch(ctx, "lsmr.u", (size_t)m, &u)) || (r = dz_scratch(ctx, "lsmr.v", (size_t)n, &v)) ||
        (r = dz_scratch(ctx, "lsmr.h", (size_t)n, &h)) || (r = dz_scratch(ctx, "lsmr.hbar", (size_t)n, &hbar)) ||
        (r = dz_scratch(ctx, "lsmr.part", (size_t)npart, &part)) || (r = dz_scratch(ctx, "lsmr.part2", (size_t)NPART * 2 + 8, &part2)) ||
        (r = dz_scratch(ctx, "lsmr.partx", (size_t)NPART, &partx)) || (r = dz_scratch(ctx, "lsmr.scal", 16, &d_scal)) ||
        (r = dz_scratch(ctx, "lsmr.state", 1, &S)))
      return r;
    if (trace && (r = dz_scratch(ctx, "lsmr.trace", (size_t)trace_cap, &d_trace))) return r;
    if (!dz_use_scatter(ctx, A) && !A->colptr && (r = dz_build_transpose(ctx, const_cast<dazim_csr *>(A)))) return r;
    // the reorthogonalisation window, sized by its upper bound min(localSize, n) (the global row count, known after the
    // consensus, can only make it smaller): allocated here so that its failure is part of the vote
    const int64_t lv = localSize < 0 ? 0 : (localSize < n ? localSize : n);
    if (lv > 0 && (r = dz_scratch(ctx, "lsmr.localV", (size_t)n * lv, &localV))) return r;
    return 0;
  }
  // after the consensus a rank that fails on its own must not leave the others waiting in a collective: abort the communicator
  // (every pending and future collective on it returns an error on every rank) and detach it
  int leave(int code) {
    if (comm) dz_comm_abort(ctx);
    comm = nullptr;
    return code;
  }
  // rc = what alloc() returned here.  Row-sharded: agree on (failure, n, m_total), every rank leaves together or none does
  int agree(int rc) {
    if (!comm) return rc;
    long long hv[4] = {rc != 0 ? 1 : 0, (long long)n, -(long long)n, 0}, *dv = d_cons;
    double hm = (double)m;
    if (!dv) return leave(rc ? rc : dz_fail(ctx, -3, "row-sharded LSMR: no memory for the consensus buffer"));
    (void)hipMemcpyAsync(dv, hv, sizeof hv, hipMemcpyHostToDevice, ctx->stream);
    (void)hipMemcpyAsync(dv + 4, &hm, 8, hipMemcpyHostToDevice, ctx->stream);
    const int r1 = dz_allreduce(ctx, comm, dv, 3, DZ_I64, DZ_MAX);
    const int r2 = dz_allreduce(ctx, comm, dv + 4, 1, DZ_F64, DZ_SUM);
    (void)hipMemcpyAsync(hv, dv, sizeof hv, hipMemcpyDeviceToHost, ctx->stream);
    (void)hipMemcpyAsync(&hm, dv + 4, 8, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    if (r1 != 0 || r2 != 0 || e != hipSuccess) return dz_fail(ctx, -2000, "row-sharded LSMR: consensus all-reduce failed");
    if (hv[0]) return dz_fail(ctx, -2001, "row-sharded LSMR: another rank failed during set-up");
    if (hv[1] != -hv[2]) return dz_fail(ctx, DAZIM_E_BAD_ARG, "row-sharded LSMR: the ranks disagree on the number of columns (%lld here, %lld elsewhere)", (long long)n, hv[1]);
    m_glob = (int64_t)hm;
    return 0;
  }
  // the reorthogonalisation window; the pinned state slots and the events
  int prepare() {
    localVecs = localSize < 0 ? 0 : localSize;
    if (m_glob < localVecs) localVecs = (int)m_glob;
    if (n < localVecs) localVecs = (int)n;
    DZ_HIP(hipHostMalloc((void **)&guard.h, sizeof(LsmrState) * (NSLOT + 1) + 64));
    h_state = guard.h;
    h_scal = (float *)(guard.h + NSLOT + 1);
    DZ_HIP(hipEventCreate(&guard.e0));
    DZ_HIP(hipEventCreate(&guard.e1));
    for (int i = 0; i < NSLOT; i++) {
      DZ_HIP(hipEventCreate(&guard.done[i]));
      for (int j = 0; j < 4; j++) DZ_HIP(hipEventCreate(&guard.ta[i][j]));
    }
    return 0;
  }
  // how k_reorth_coop would cover v (a function of n alone), and whether the device can hold that launch
  void plan_reorth() {
    // the grid barrier of k_reorth_coop needs every workgroup resident at once: bounded by what the occupancy query allows on this
    // device (taken once per solve) -- never on a stream restricted to some CUs (DAZIM_CU_MASK), where that bound does not hold
    if (!getenv("DAZIM_CU_MASK")) {
      int occ = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_reorth_coop<16>, RC_THREADS, 0) == hipSuccess && occ > 0) coop_max = occ * ctx->num_cu;
      else (void)hipGetLastError();
    }
    // as few workgroups as hold v with <= RC_EMAX elements per thread, eight where that is enough: a step's grid barrier is
    // atomics on one word across XCDs (whose L2s do not share it), and its cost grows with the arrivals -- test4_Yunnan's
    // 73 440-float v, ten vectors: 52 us with 64 workgroups (= the chain's eleven launches), 33 us with 8
    rcb = (int)((n + (int64_t)RC_THREADS * RC_EMAX - 1) / ((int64_t)RC_THREADS * RC_EMAX));
    if (rcb < 8) rcb = 8;
    if (rcb > (int)((n + RC_THREADS - 1) / RC_THREADS)) rcb = (int)((n + RC_THREADS - 1) / RC_THREADS);
    if (rcb > RC_BLOCKS) rcb = RC_BLOCKS;
    per_thread = (n + (int64_t)rcb * RC_THREADS - 1) / ((int64_t)rcb * RC_THREADS);
  }
  // rowwise = the vector is sharded by rows (u): its squared norm is summed over the ranks first
  int norm_to_host(const double *pp, int np, float *res, bool rowwise = false) {
    if (comm && rowwise) {
      hipLaunchKernelGGL(finish_norm, dim3(1), dim3(64), 0, ctx->stream, pp, np, d_scal, d_sum);
      if (const int rr = dz_allreduce(ctx, comm, d_sum, 1, DZ_F64, DZ_SUM)) return rr;
      hipLaunchKernelGGL(k_sqrt_sum, dim3(1), dim3(1), 0, ctx->stream, d_sum, d_scal);
    } else {
      hipLaunchKernelGGL(finish_norm, dim3(1), dim3(64), 0, ctx->stream, pp, np, d_scal, (double *)nullptr);
    }
    DZ_HIP(hipMemcpyAsync(h_scal, d_scal, 4, hipMemcpyDeviceToHost, ctx->stream));
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    *res = h_scal[0];
    return 0;
  }
  // v(out) = A^T u + sign*beta*v with partials of ||v||^2 in `part` (row-sharded: local product, all-reduce, then the axpby)
  int spmvT(const float *beta_p, float sign, const int *g) {
    if (!comm) return dz_launch_spmvT(ctx, A, u, ymax, v, beta_p, sign, part, &gn_t, g);
    DZ_HIP(hipMemsetAsync(wbuf, 0, n * 4, ctx->stream));
    if (const int r = dz_launch_spmvT(ctx, A, u, ymax, wbuf, nullptr, 1.0f, nullptr, nullptr, g)) return r;
    if (const int rr = dz_allreduce(ctx, comm, wbuf, (size_t)n, DZ_F32, DZ_SUM)) return rr;
    hipLaunchKernelGGL(k_axpby_norm, dim3(bn), dim3(VB), 0, ctx->stream, n, wbuf, v, beta_p, sign, part, g);
    gn_t = bn;
    return 0;
  }
  // u = b ; beta = ||u|| ; u /= beta ; v = A^T u ; alpha = ||v|| ; v /= alpha   (:355-372), the initial state, trace record 0
  int start() {
    int rc;
    DZ_HIP(hipEventRecord(guard.e0, ctx->stream));
    hipLaunchKernelGGL(k_copy, dim3(bm), dim3(VB), 0, ctx->stream, m, b.dev, u);
    DZ_HIP(hipMemsetAsync(v, 0, n * 4, ctx->stream));
    DZ_HIP(hipMemsetAsync(x.dev, 0, n * 4, ctx->stream));
    DZ_HIP(hipMemsetAsync(hbar, 0, n * 4, ctx->stream));
    hipLaunchKernelGGL(k_sumsq, dim3(bm), dim3(VB), 0, ctx->stream, m, u, part);
    float alpha = 0.0f, beta = 0.0f;
    if ((rc = norm_to_host(part, bm, &beta, true))) return rc;
    if (!std::isfinite(beta)) ymax = beta;
    if (beta > 0.0f) {
      hipLaunchKernelGGL(k_scal_inv, dim3(bm), dim3(VB), 0, ctx->stream, m, u, d_scal, 1.0f);
      if ((rc = spmvT(nullptr, 1.0f, nullptr))) return rc;  // v = 1*v(=0) + A^T u
      if ((rc = norm_to_host(part, gn_t, &alpha))) return rc;
    }
    if (alpha > 0.0f) hipLaunchKernelGGL(k_scal_inv, dim3(bn), dim3(VB), 0, ctx->stream, n, v, d_scal, 1.0f);
    normAr = alpha * beta;
    normb = beta;
    if (trace) {   // the line the reference prints before the loop (:468-471): itn 0, x(1) = 0, test1 = 1, test2 = alpha/beta
      memset(&trace[0], 0, sizeof trace[0]);
      trace[0].normr = beta; trace[0].normAr = normAr; trace[0].test1 = 1.0f; trace[0].test2 = beta > 0.0f ? alpha / beta : 0.0f;
      ntrace = 1;
    }
    if (normAr == 0.0f) return 0;   // x = 0 solves the system: run() has nothing to do
    if (localVecs > 0) hipLaunchKernelGGL(k_copy, dim3(bn), dim3(VB), 0, ctx->stream, n, v, localV);   // localV(:,1) = v
    hipLaunchKernelGGL(k_copy, dim3(bn), dim3(VB), 0, ctx->stream, n, v, h);
    LsmrState &s0 = h_state[NSLOT];
    memset(&s0, 0, sizeof s0);
    s0.alpha = alpha; s0.beta = beta; s0.alphabar = alpha; s0.zetabar = alpha * beta; s0.rho = 1; s0.rhobar = 1; s0.cbar = 1;
    s0.betadd = beta; s0.rhodold = 1; s0.normA2 = alpha * alpha; s0.minrbar = 1e+30f; s0.normb = beta;
    s0.ctol = conlim > 0.0f ? 1.0f / conlim : 0.0f;
    s0.normr = beta; s0.normAr = normAr; s0.damp = damp; s0.atol = atol; s0.btol = btol; s0.itnlim = itnlim;
    DZ_HIP(hipMemcpyAsync(S, &s0, sizeof s0, hipMemcpyHostToDevice, ctx->stream));
    if (d_trace) DZ_HIP(hipMemsetAsync(d_trace, 0, (size_t)trace_cap * sizeof(dazim_lsmr_rec), ctx->stream));
    g1 = &S->stop;
    g2 = &S->stop2;
    plan_reorth();
    rccl_allreduce = comm && comm->nccl && dz_opt(ctx, "comm.allreduce", 0) == 1;
    DZ_HIP(hipMemsetAsync(part2 + 2 * NPART, 0, 64, ctx->stream));
    return 0;
  }
  // first half-step: u = A v - alpha u (:484-486) with the partials of ||u||^2
  int half_step_u(hipEvent_t *tev) {
    if (tev) DZ_HIP(hipEventRecord(tev[0], ctx->stream));
    if (const int r = dz_launch_spmvA(ctx, A, v, u, &S->alpha, -1.0f, part, &gm_t, g1)) return r;
    if (tev) DZ_HIP(hipEventRecord(tev[1], ctx->stream));
    return 0;
  }
  // second half-step: beta = ||u||, u /= beta, v -> slot of the window, v = A^T u - beta v (:487-497) with the partials of ||v||^2
  int half_step_v(float *slot, hipEvent_t *tev) {
    int r;
    if (!comm) {
      hipLaunchKernelGGL(k_beta_scal_u, dim3(bm > bn ? bm : bn), dim3(VB), 0, ctx->stream, m, u, part, gm_t,
                         (const double *)nullptr, n, v, slot, S);
      if (tev) DZ_HIP(hipEventRecord(tev[2], ctx->stream));
      if ((r = spmvT(&S->beta, -1.0f, g2))) return r;                                     // v = A^T u - beta v (:496-497)
      if (tev) DZ_HIP(hipEventRecord(tev[3], ctx->stream));
      return 0;
    }
    // row-sharded: ONE collective per iteration (see k_local_norm_scal / k_beta_axpby)
    float *d_bp = reinterpret_cast<float *>(d_sum + 4);
    double *w_sum = reinterpret_cast<double *>(reinterpret_cast<char *>(wbuf) + w_sum_off);
    const int bmn = bm > bn ? bm : bn;
    hipLaunchKernelGGL(k_local_norm_scal, dim3(bm), dim3(VB), 0, ctx->stream, m, u, part, gm_t, w_sum, d_bp, S);
    if (tev) DZ_HIP(hipEventRecord(tev[2], ctx->stream));
    DZ_HIP(hipMemsetAsync(wbuf, 0, n * 4, ctx->stream));
    if ((r = dz_launch_spmvT(ctx, A, u, ymax, wbuf, nullptr, 1.0f, nullptr, nullptr, g1))) return r;
    hipLaunchKernelGGL(k_scale_by, dim3(bn), dim3(VB), 0, ctx->stream, n, wbuf, d_bp, g1);
    if (tev) DZ_HIP(hipEventRecord(tev[3], ctx->stream));
    if (rccl_allreduce) {   // option comm.allreduce: RCCL's own sums (its order), the two buffers in one group
      DZ_NCCL(ncclGroupStart());
      const ncclResult_t ra = ncclAllReduce(wbuf, wbuf, (size_t)n, ncclFloat, ncclSum, comm->nccl, ctx->stream);
      const ncclResult_t rb = ncclAllReduce(w_sum, w_sum, 1, ncclDouble, ncclSum, comm->nccl, ctx->stream);
      const ncclResult_t rg = ncclGroupEnd();   // (inside a group the calls above only enqueue: launch errors surface here)
      if (ra != ncclSuccess || rb != ncclSuccess || rg != ncclSuccess) {
        const ncclResult_t bad = ra != ncclSuccess ? ra : (rb != ncclSuccess ? rb : rg);
        return dz_fail(ctx, -2000 - (int)bad, "row-sharded LSMR: grouped ncclAllReduce -> %s", ncclGetErrorString(bad));
      }
      hipLaunchKernelGGL(k_beta_axpby, dim3(bmn), dim3(VB), 0, ctx->stream, m, u, n, v, (const char *)wbuf, 1, w_bytes, w_sum_off, d_bp,
                         slot, part, S);
    } else {
      if ((r = dz_allgather(ctx, comm, wbuf, gbuf, w_bytes))) return r;
      hipLaunchKernelGGL(k_beta_axpby, dim3(bmn), dim3(VB), 0, ctx->stream, m, u, n, v, (const char *)gbuf, comm->nranks, w_bytes,
                         w_sum_off, d_bp, slot, part, S);
    }
    n_coll++;
    gn_t = bmn;
    return 0;
  }
  // localVOrtho :733-748 over the lim vectors of the window; returns how many partials in `part` now hold ||v||^2
  int reorthogonalise(int lim) {
    // in one launch (k_reorth_coop) when v fits the registers of workgroups that are all resident at once (see plan_reorth())
    if (localVecs > 0 && lim > 0 && per_thread <= RC_EMAX && rcb <= coop_max) {
      unsigned *bar = reinterpret_cast<unsigned *>(part2 + 2 * NPART);
      const unsigned base = reorth_barriers;
      reorth_barriers += (unsigned)lim * (unsigned)rcb;
#define DZ_RC(E_) hipLaunchKernelGGL(k_reorth_coop<E_>, dim3(rcb), dim3(RC_THREADS), 0, ctx->stream, n, v, localV, lim, part2, part, bar, base, g2)
      if (per_thread <= 1) DZ_RC(1); else if (per_thread <= 2) DZ_RC(2); else if (per_thread <= 4) DZ_RC(4); else if (per_thread <= 8) DZ_RC(8); else DZ_RC(16);
#undef DZ_RC
      return rcb;
    }
    if (localVecs > 0) {   // ... or as the chain: modified Gram-Schmidt, one launch per vector; the last one leaves ||v||^2
      for (int q = 0; q <= lim; q++) {
        const float *prev = q > 0 ? localV + (size_t)(q - 1) * n : nullptr;
        const float *next = q < lim ? localV + (size_t)q * n : nullptr;
        hipLaunchKernelGGL(k_reorth, dim3(bn), dim3(VB), 0, ctx->stream, n, v, prev, part2 + ((q + 1) & 1) * NPART, bn, next,
                           q < lim ? part2 + (q & 1) * NPART : part, g2);
      }
      return bn;
    }
    return gn_t;   // no window: the partials of the product
  }
  // one iteration, enqueued without any host synchronisation; k = its number (the reorthogonalisation window is a function
  // of k alone: localVEnqueue advances once per iteration, :723-731)
  int enqueue_iteration(int k, hipEvent_t *tev) {
    int r;
    if ((r = half_step_u(tev))) return r;
    float *slot = nullptr;
    int lim = 0;
    if (localVecs > 0) {
      const int ptr = k % localVecs + 1;             // localPointer after this iteration's enqueue
      slot = localV + (size_t)(ptr - 1) * n;
      lim = k >= localVecs ? localVecs : k + 1;     // localVQueueFull ? localVecs : localPointer (:738-742)
    }
    if ((r = half_step_v(slot, tev))) return r;
    const int npa = reorthogonalise(lim);
    hipLaunchKernelGGL(k_alpha_update, dim3(bn), dim3(VB), 0, ctx->stream, n, v, h, hbar, x.dev, part, npa, partx, S);
    hipLaunchKernelGGL(k_tests, dim3(1), dim3(64), 0, ctx->stream, partx, bn, x.dev, S, d_trace, trace_cap);
    DZ_HIP(hipGetLastError());
    return 0;
  }
  // batches of CHECK iterations; the state after batch j is copied to pinned slot j % NSLOT and examined while batch j+1
  // is already running
  int run() {
    if (normAr == 0.0f) return 0;   // (start() found x = 0)
    int rc;
    LsmrState &s0 = h_state[NSLOT];
    const int limit = itnlim > 1 ? itnlim : 1;   // (the reference tests itn >= itnlim after its first iteration)
    int launched = 0, nbatch = 0, examined = 0;
    bool stopped = false;
    while (!stopped) {
      if (launched < limit) {
        const int sl = nbatch % NSLOT;
        for (int i = 0; i < CHECK && launched < limit; i++) {
          launched++;
          n_enq++;
          if ((rc = enqueue_iteration(launched, i == 0 ? guard.ta[sl] : nullptr))) return rc;
        }
        DZ_HIP(hipMemcpyAsync(&h_state[sl], S, sizeof(LsmrState), hipMemcpyDeviceToHost, ctx->stream));
        DZ_HIP(hipEventRecord(guard.done[sl], ctx->stream));
        nbatch++;
      }
      const int keep = launched < limit ? 1 : 0;   // one batch stays unexamined while more can be enqueued behind it
      while (examined < nbatch - keep && !stopped) {
        const int ls = examined % NSLOT;
        DZ_HIP(hipEventSynchronize(guard.done[ls]));
        host_syncs++;
        float ms = 0;
        if (hipEventElapsedTime(&ms, guard.ta[ls][0], guard.ta[ls][1]) == hipSuccess) { t_spmv += ms * 1e-3; n_spmv++; }
        if (hipEventElapsedTime(&ms, guard.ta[ls][2], guard.ta[ls][3]) == hipSuccess) { t_spmvt += ms * 1e-3; n_spmvt++; }
        s0 = h_state[ls];
        stopped = s0.stop != 0;
        examined++;
      }
      if (!stopped && launched >= limit && examined == nbatch) stopped = true;   // (istop = 7 sets the flag at itn >= itnlim)
    }
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    istop = s0.istop; itn = s0.itn; normA = s0.normA; condA = s0.condA; normr = s0.normr; normAr = s0.normAr; normx = s0.normx;
    if (trace) {
      const int cnt = itn + 1 < trace_cap ? itn + 1 : trace_cap;
      if (cnt > 1) {
        DZ_HIP(hipMemcpyAsync(trace + 1, d_trace + 1, (size_t)(cnt - 1) * sizeof(dazim_lsmr_rec), hipMemcpyDeviceToHost, ctx->stream));
        DZ_HIP(hipStreamSynchronize(ctx->stream));
      }
      ntrace = cnt;
    }
    return 0;
  }
  // the solve's timings and counts, the output arguments, x
  int report() {
    int rc;
    if (damp > 0.0f && istop == 2) istop = 3;  // :686
    DZ_HIP(hipEventRecord(guard.e1, ctx->stream));
    DZ_HIP(hipEventSynchronize(guard.e1));
    float ms = 0;
    DZ_HIP(hipEventElapsedTime(&ms, guard.e0, guard.e1));
    ctx->ksec["lsmr"] = ms * 1e-3;
    ctx->ksec["spmv"] = n_spmv ? t_spmv / n_spmv : -1.0;
    ctx->ksec["spmvt"] = n_spmvt ? t_spmvt / n_spmvt : -1.0;
    ctx->ksec["lsmr.normb"] = normb;
    ctx->ksec["lsmr.host_syncs"] = host_syncs;
    // the form reorthogonalise() took (the same for every iteration of a solve): 0 no window (or no iteration), 1 k_reorth_coop, 2 the chain
    ctx->ksec["lsmr.reorth_kind"] = localVecs > 0 && n_enq > 0 ? (per_thread <= RC_EMAX && rcb <= coop_max ? 1.0 : 2.0) : 0.0;
    ctx->ksec["lsmr.reorth_blocks"] = rcb;
    ctx->ksec["lsmr.reorth_per_thread"] = (double)per_thread;
    // counted, not assumed: collectives issued by the loop / iterations enqueued (the n floats of A_p^T u_p with the double ||u_p||^2)
    ctx->ksec["lsmr.collectives_per_iteration"] = comm && n_enq > 0 ? (double)n_coll / (double)n_enq : 0.0;
    ctx->ksec["lsmr.collective_kind"] = comm ? (rccl_allreduce ? 2.0 : 1.0) : 0.0;   // 1 all-gather + rank-ordered sums, 2 ncclAllReduce
    {
      int nr = 1;
      if (comm && comm->nccl) (void)ncclCommCount(comm->nccl, &nr);
      else if (comm) nr = comm->nranks;
      ctx->ksec["lsmr.nranks"] = nr;     // ranks the communicator of this solve really has
      ctx->ksec["lsmr.transport"] = comm ? (comm->nccl ? 1.0 : 2.0) : 0.0;   // 1 RCCL, 2 files (tests)
    }
    if (istop_o) *istop_o = istop;
    if (itn_o) *itn_o = itn;
    if (normA_o) *normA_o = normA;
    if (condA_o) *condA_o = condA;
    if (normr_o) *normr_o = normr;
    if (normAr_o) *normAr_o = normAr;
    if (normx_o) *normx_o = normx;
    if (trace_n) *trace_n = ntrace;
    if ((rc = x.finish())) return rc;
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
  }
};

}  // namespace

extern "C" {

// LSMR, inv/lsmrModule.f90:36-750.  Vectors AND scalars live on the device (LsmrState above); the host enqueues
// iterations and looks at the stop flag every CHECK iterations, one batch behind the one being enqueued, so the GPU never waits
// for the host.  With a communicator attached (dazim_comm_init) A and b are this rank's rows of one global system: one collective
// per iteration carries the n floats of A_p^T u_p and the double ||u_p||^2, the state is replicated.
int dazim_lsmr_traced(dazim_ctx *ctx, const dazim_csr *A, const float *b_u, float damp, float atol, float btol,
                      float conlim, int itnlim, int localSize, float *x_u, int *istop_o, int *itn_o,
                      float *normA_o, float *condA_o, float *normr_o, float *normAr_o, float *normx_o,
                      dazim_lsmr_rec *trace, int trace_cap, int *trace_n) {
  if (!ctx || !A || !b_u || !x_u || (trace && trace_cap < 1)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_lsmr");
  DZ_HIP(hipSetDevice(ctx->device));
  LsmrSolve s(LsmrArgs{ctx, A, b_u, damp, atol, btol, conlim, itnlim, localSize, x_u, istop_o, itn_o, normA_o, condA_o, normr_o,
                       normAr_o, normx_o, trace, trace_cap, trace_n});
  int rc = s.agree(s.alloc());
  if (rc) return rc;   // (a failed vote leaves the communicator alone: every rank returns here)
  // ---- from here on a local failure (a launch, a copy, a collective) aborts the communicator: see LsmrSolve::leave ----
  if ((rc = s.prepare()) || (rc = s.start()) || (rc = s.run()) || (rc = s.report())) return s.leave(rc);
  return 0;
}

int dazim_lsmr(dazim_ctx *ctx, const dazim_csr *A, const float *b_u, float damp, float atol, float btol,
               float conlim, int itnlim, int localSize, float *x_u, int *istop_o, int *itn_o,
               float *normA_o, float *condA_o, float *normr_o, float *normAr_o, float *normx_o) {
  return dazim_lsmr_traced(ctx, A, b_u, damp, atol, btol, conlim, itnlim, localSize, x_u, istop_o, itn_o, normA_o, condA_o,
                           normr_o, normAr_o, normx_o, nullptr, 0, nullptr);
}

}  // extern "C"
