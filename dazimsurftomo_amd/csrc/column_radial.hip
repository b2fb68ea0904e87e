// column_radial.hip -- radial anisotropy in the second step of the two-step method: Vsv from the Rayleigh
// maps and Vsh from the Love maps of one cell, two profiles of n knots each, tied by a prior towards isotropy.
//
// dazim_column_lsq_radial: per inner cell the unknowns x = [xv; xh] (N = 2n <= 126) of
//   min ||Wv (Kv xv - rv)||^2 + ||Wh (Kh xh - rh)||^2 + s2 (||L xv||^2 + ||L xh||^2) + d2 ||x||^2 + m2 ||xh - xv + d0||^2
// by the normal equations A x = b,
//   A = [[Kv^T Wv^2 Kv + P + m2 I, -m2 I], [-m2 I, Kh^T Wh^2 Kh + P + m2 I]],  P = s2 L^T L + d2 I,
//   b = [Kv^T Wv^2 rv + m2 d0; Kh^T Wh^2 rh - m2 d0],
// and the Cholesky factor A = R R^T.  One workgroup per cell, lane = row of A (64 lanes up to N = 64, 128 beyond), fp64, every sum
// in a fixed order: the same inputs give the same bits, from the host or the device.  With m2 = 0 the cross block of R stays 0 and
// each diagonal block runs through the operations of dz_column_solve on that block alone.
// dazim_column_resolution_radial: C = A^-1 and Rm = I - C P2, P2 = [[P + m2 I, -m2 I], [-m2 I, P + m2 I]], from the same factor
// (cr_assemble_factor serves both kernels): M = R^-1 in place, then C = M^T M in place (potrf -> trtri -> lauum).
// LDS: a full A [126][126] beside K and a row-per-lane copy of C does not fit in 160 KiB, so A is the packed lower triangle, row a at
// a (a + 1) / 2: N (N + 1) / 2 doubles (64 008 bytes at N = 126), then K [kv + kh][n], w^2 [kv + kh], w^2 r [kv + kh] and b [N]
// (right-hand side, then solution; the resolution kernel keeps the lanes' Rm_aa there): 8 (N (N + 1) / 2 + (kv + kh)(n + 2) + N)
// bytes, 96 216 at n = 63, kv + kh = 60 and 3 376 at n = 10, kv + kh = 16, sized by the call's own n, kv, kh.
#include "dazim_internal.h"

#include <cmath>

namespace {

constexpr int CR_MAXLAY = 63, CR_MAXPER = 60;

__device__ __forceinline__ int cr_tri(int a, int c) { return a * (a + 1) / 2 + c; }   // (a, c) of the packed lower triangle, c <= a

struct CrLds {
  double *A, *K, *w2, *wr, *b;
};
__device__ __forceinline__ CrLds cr_carve(double *sm, int n, int kt) {
  CrLds L;
  L.A = sm;
  L.K = L.A + n * (2 * n + 1);
  L.w2 = L.K + kt * n;
  L.wr = L.w2 + kt;
  L.b = L.wr + kt;
  return L;
}
size_t cr_lds_bytes(int n, int kt) { return ((size_t)n * (2 * n + 1) + (size_t)kt * (n + 2) + 2 * (size_t)n) * sizeof(double); }

// The cell's weights (lane p < kv: Rayleigh period p; kv <= p < kv + kh: Love period p - kv), with rhs its w^2 r, and its kernels:
// K [kv + kh][n], the Rayleigh rows first.  Returns whether any weight is not 0 (the same on every lane); without one nothing else
// is read.  Ends on a barrier.
__device__ __forceinline__ bool cr_load(int t, int n, int kv, int kh, long ncol, long col, int ncell, int cell,
                                        const double *__restrict__ kern_v, const double *__restrict__ kern_h,
                                        const float *__restrict__ w_v, const float *__restrict__ w_h,
                                        const float *__restrict__ rhs_v, const float *__restrict__ rhs_h, const CrLds &L) {
  bool data = false;
  if (t < kv + kh) {
    const bool h = t >= kv;
    const long o = (long)(h ? t - kv : t) * ncell + cell;
    const float *wd = h ? w_h : w_v;
    const float w = wd ? wd[o] : 1.0f;
    data = w != 0.0f;
    const double ww = (double)w * (double)w;
    L.w2[t] = ww;
    if (rhs_v || rhs_h) L.wr[t] = data ? ww * (double)(h ? rhs_h : rhs_v)[o] : 0.0;
  }
  if (!__syncthreads_or(data)) return false;
  for (int q = t; q < n * kv; q += blockDim.x) {   // q = l*kv + p, the table's own order
    const int l = q / kv, p = q - l * kv;
    L.K[p * n + l] = kern_v[(long)q * ncol + col];
  }
  for (int q = t; q < n * kh; q += blockDim.x) {
    const int l = q / kh, p = q - l * kh;
    L.K[(kv + p) * n + l] = kern_h[(long)q * ncol + col];
  }
  __syncthreads();
  return true;
}

// Lane t < 2n builds row t of A (its packed lower part) from K and w^2, then all factor it: right-looking Cholesky, column by
// column, each lane updating its own row.  R replaces A.  Returns whether every pivot was finite and > 0 (the same on every
// lane); the arithmetic does not depend on it.  The caller has passed a barrier after filling K and w2.
__device__ __forceinline__ bool cr_assemble_factor(int t, int n, int kv, int kh, double *A, const double *K, const double *w2,
                                                   double s2, double d2, double m2) {
  const int N = 2 * n;
  if (t < N) {
    const int blk = t >= n, ka = t - blk * n, kb = blk ? kh : kv;
    const double *Kb = K + (blk ? kv * n : 0), *wb = w2 + (blk ? kv : 0);
    double *row = A + cr_tri(t, 0);
    if (blk)
      for (int c = 0; c < n; c++) row[c] = c == ka ? -m2 : 0.0;
    row += blk * n;
    for (int c = 0; c <= ka; c++) {
      double s = 0.0;
      for (int p = 0; p < kb; p++)
        if (wb[p] != 0.0) s += wb[p] * Kb[p * n + ka] * Kb[p * n + c];
      s += s2 * dz_ltl(n, ka, c);
      if (c == ka) {
        s += d2;
        s += m2;
      }
      row[c] = s;
    }
  }
  __syncthreads();
  bool ok = true;
  for (int c = 0; c < N; c++) {
    const double p = A[cr_tri(c, c)];
    ok = ok && isfinite(p) && p > 0.0;
    const double d = sqrt(p);
    if (t > c && t < N) A[cr_tri(t, c)] /= d;
    __syncthreads();
    if (t == c) A[cr_tri(c, c)] = d;
    if (t > c && t < N) {
      double *row = A + cr_tri(t, 0);
      const double f = row[c];
      for (int e = c + 1; e <= t; e++) row[e] -= f * A[cr_tri(e, c)];
    }
    __syncthreads();
  }
  return ok;
}

__global__ void k_column_lsq_radial(int nx, int ny, int n, int kv, int kh, const double *__restrict__ kern_v,
                                    const double *__restrict__ kern_h, const float *__restrict__ rhs_v,
                                    const float *__restrict__ rhs_h, const float *__restrict__ w_v, const float *__restrict__ w_h,
                                    const float *__restrict__ d0, double s2, double d2, double m2, float *__restrict__ x,
                                    int *__restrict__ n_empty, double *__restrict__ part) {
  extern __shared__ double sm[];
  const int kt = kv + kh, N = 2 * n;
  const CrLds L = cr_carve(sm, n, kt);
  const int t = threadIdx.x;
  const int nvx = nx - 2, ncell = nvx * (ny - 2);
  const int cell = blockIdx.x;
  const int j = cell / nvx, i = cell - j * nvx;
  const long ncol = (long)nx * ny, col = (long)(j + 1) * nx + (i + 1);

  if (!cr_load(t, n, kv, kh, ncol, col, ncell, cell, kern_v, kern_h, w_v, w_h, rhs_v, rhs_h, L)) {   // no data: x = 0 exactly
    if (t < N) x[(long)t * ncell + cell] = 0.0f;
    if (part && t < kt) {
      const long o = ((long)t * ncell + cell) * 2;
      part[o] = 0.0;
      part[o + 1] = 0.0;
    }
    if (t == 0) atomicAdd(n_empty, 1);
    return;
  }
  if (t < N) {                                    // b = K^T W^2 r +- m2 d0
    const int blk = t >= n, ka = t - blk * n, kb = blk ? kh : kv;
    const double *Kb = L.K + (blk ? kv * n : 0), *wb = L.w2 + (blk ? kv : 0), *rb = L.wr + (blk ? kv : 0);
    double s = 0.0;
    for (int p = 0; p < kb; p++)
      if (wb[p] != 0.0) s += rb[p] * Kb[p * n + ka];
    const double md = d0 ? m2 * (double)d0[(long)ka * ncell + cell] : 0.0;
    L.b[t] = blk ? s - md : s + md;
  }
  cr_assemble_factor(t, n, kv, kh, L.A, L.K, L.w2, s2, d2, m2);
  for (int c = 0; c < N; c++) {                   // R y = b
    const double y = L.b[c] / L.A[cr_tri(c, c)];
    __syncthreads();
    if (t > c && t < N) L.b[t] -= L.A[cr_tri(t, c)] * y;
    if (t == c) L.b[c] = y;
    __syncthreads();
  }
  for (int c = N - 1; c >= 0; c--) {              // R^T x = y
    const double y = L.b[c] / L.A[cr_tri(c, c)];
    __syncthreads();
    if (t < c) L.b[t] -= L.A[cr_tri(c, t)] * y;
    if (t == c) L.b[c] = y;
    __syncthreads();
  }
  if (t < N) x[(long)t * ncell + cell] = (float)L.b[t];
  if (part && t < kt) {                           // r^2 and (r - K x)^2 of this cell, 0 where w = 0
    double rr = 0.0, ee = 0.0;
    if (L.w2[t] != 0.0) {
      const bool h = t >= kv;
      const double rv = (double)(h ? rhs_h : rhs_v)[(long)(h ? t - kv : t) * ncell + cell];
      const double *xb = L.b + (h ? n : 0);
      double kx = 0.0;
      for (int l = 0; l < n; l++) kx += L.K[t * n + l] * xb[l];
      rr = rv * rv;
      ee = (rv - kx) * (rv - kx);
    }
    const long o = ((long)t * ncell + cell) * 2;
    part[o] = rr;
    part[o + 1] = ee;
  }
}

// Posterior of k_column_lsq_radial's problem, lane a = row a of C and of Rm (a < n: Vsv knot a; a >= n: Vsh knot a - n).  After
// cr_assemble_factor: M = R^-1 in place, column j from the last to the first, M_ij = -(sum_{l = j+1..i} M_il R_lj) / R_jj in ascending
// l (lane i; the column is written after a barrier, since lane i reads R_lj of the lanes l <= i); C = M^T M in place, row a from the
// first to the last, C_ac = sum_{i >= a} M_ia M_ic in ascending i (lane c <= a; rows >= a still hold M).  Then lane a walks its row
// of the symmetric C once: Rm_ac from the entries of column c of P2, the five of the pentadiagonal P + m2 I in c's block in
// ascending order and then -m2 at the same knot of the other block.
// cnt[0] counts the cells without data (every output 0), cnt[1] those with a pivot that is not finite and > 0 (every output NaN).
__global__ void k_column_res_radial(int nx, int ny, int n, int kv, int kh, const double *__restrict__ kern_v,
                                    const double *__restrict__ kern_h, const float *__restrict__ w_v, const float *__restrict__ w_h,
                                    double s2, double d2, double m2, float *__restrict__ std_post, float *__restrict__ cov_vh,
                                    float *__restrict__ rdiag, float *__restrict__ rsum, float *__restrict__ cross,
                                    float *__restrict__ trace, float *__restrict__ rows, int *__restrict__ cnt) {
  extern __shared__ double sm[];
  const int kt = kv + kh, N = 2 * n;
  const CrLds L = cr_carve(sm, n, kt);
  double *A = L.A;
  const int t = threadIdx.x;
  const int nvx = nx - 2, ncell = nvx * (ny - 2);
  const int cell = blockIdx.x;
  const int j = cell / nvx, i = cell - j * nvx;
  const long ncol = (long)nx * ny, col = (long)(j + 1) * nx + (i + 1);
  const long o = (long)t * ncell + cell;

  auto fill = [&](float v) {                      // every output of this cell = v
    if (t < N) std_post[o] = rdiag[o] = rsum[o] = cross[o] = v;
    if (t < n) cov_vh[o] = v;
    if (trace && t < 2) trace[o] = v;
    if (rows)
      for (int q = t; q < N * N; q += blockDim.x) rows[(long)q * ncell + cell] = v;
  };
  if (!cr_load(t, n, kv, kh, ncol, col, ncell, cell, kern_v, kern_h, w_v, w_h, nullptr, nullptr, L)) {
    fill(0.0f);
    if (t == 0) atomicAdd(cnt, 1);
    return;
  }
  if (!cr_assemble_factor(t, n, kv, kh, A, L.K, L.w2, s2, d2, m2)) {
    fill(nanf(""));
    if (t == 0) atomicAdd(cnt + 1, 1);
    return;
  }
  for (int c = N - 1; c >= 0; c--) {              // M = R^-1
    const double inv = 1.0 / A[cr_tri(c, c)];
    double v = 0.0;
    if (t > c && t < N) {
      const double *row = A + cr_tri(t, 0);
      double s = 0.0;
      for (int l = c + 1; l <= t; l++) s += row[l] * A[cr_tri(l, c)];
      v = -s * inv;
    }
    __syncthreads();
    if (t > c && t < N) A[cr_tri(t, c)] = v;
    if (t == c) A[cr_tri(c, c)] = inv;
    __syncthreads();
  }
  for (int a = 0; a < N; a++) {                   // C = M^T M
    double s = 0.0;
    if (t <= a)
      for (int q = a; q < N; q++) s += A[cr_tri(q, a)] * A[cr_tri(q, t)];
    __syncthreads();
    if (t <= a) A[cr_tri(a, t)] = s;
    __syncthreads();
  }
  double rd = 0.0;
  if (t < N) {
    const int a = t, blk = a >= n;
    auto C = [&](int e) { return e <= a ? A[cr_tri(a, e)] : A[cr_tri(e, a)]; };
    double rs = 0.0, other = 0.0, all = 0.0;
    for (int c = 0; c < N; c++) {
      const int cb = c >= n, kc = c - cb * n;
      double s = 0.0;
      for (int e = max(kc - 2, 0); e <= min(kc + 2, n - 1); e++) s += C(cb * n + e) * (s2 * dz_ltl(n, e, kc) + (e == kc ? d2 + m2 : 0.0));
      s -= C(cb ? kc : kc + n) * m2;
      const double rm = (a == c ? 1.0 : 0.0) - s;
      if (rows) rows[((long)a * N + c) * ncell + cell] = (float)rm;
      rs += rm;
      all += fabs(rm);
      if (cb != blk) other += fabs(rm);
      if (c == a) rd = rm;
    }
    std_post[o] = (float)sqrt(C(a));
    if (!blk) cov_vh[o] = (float)C(a + n);
    rdiag[o] = (float)rd;
    rsum[o] = (float)rs;
    cross[o] = all > 0.0 ? (float)(other / all) : 0.0f;
  }
  if (trace) {
    if (t < N) L.b[t] = rd;
    __syncthreads();
    if (t < 2) {
      double s = 0.0;
      for (int a = 0; a < n; a++) s += L.b[t * n + a];
      trace[o] = (float)s;
    }
  }
}

// what both entries refuse alike
int cr_check(dazim_ctx *ctx, const char *who, int nx, int ny, int nlay, int kv, const void *kern_v, int kh, const void *kern_h,
             float smooth, float damp, float couple) {
  if (nx < 3 || ny < 3) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: grid %d x %d has no inner cell", who, nx, ny);
  if (nlay < 1 || nlay > CR_MAXLAY) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: nlay %d outside 1..%d", who, nlay, CR_MAXLAY);
  if (kv < 0 || kh < 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: negative period count kv %d, kh %d", who, kv, kh);
  if (kv + kh < 1 || kv + kh > CR_MAXPER) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: kv + kh = %d outside 1..%d", who, kv + kh, CR_MAXPER);
  if (!(smooth >= 0.0f) || !(damp >= 0.0f) || !(couple >= 0.0f))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: negative smoothing, damping or coupling", who);
  if (smooth == 0.0f && damp == 0.0f) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: smoothing and damping both 0", who);
  if ((kv > 0) != (kern_v != nullptr) || (kh > 0) != (kern_h != nullptr))
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: a kernel table goes with a period count that is not 0 (kern_v with kv, kern_h with kh)", who);
  return 0;
}

}  // namespace

extern "C" {

int dazim_column_lsq_radial(dazim_ctx *ctx, int nx, int ny, int nlay, int kv, const double *kern_v_u, int kh, const double *kern_h_u,
                            const float *rhs_v_u, const float *rhs_h_u, const float *w_v_u, const float *w_h_u, const float *d0_u,
                            float smooth, float damp, float couple, float *x_u, int *n_empty, float *stats) {
  if (!ctx) return DAZIM_E_BAD_ARG;
  int rc;
  if ((rc = cr_check(ctx, "dazim_column_lsq_radial", nx, ny, nlay, kv, kern_v_u, kh, kern_h_u, smooth, damp, couple))) return rc;
  if ((kv > 0 && !rhs_v_u) || (kh > 0 && !rhs_h_u)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_lsq_radial: a right-hand side is missing");
  if (!x_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_lsq_radial: the output x is missing");
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (nx - 2) * (ny - 2), kt = kv + kh;
  const size_t ncol = (size_t)nx * ny;
  DzBuf<double> kvb, khb;
  DzBuf<float> rv, rh, wv, wh, d0, x;
  if ((rc = kvb.init(ctx, kern_v_u, (size_t)nlay * kv * ncol, true, false)) || (rc = khb.init(ctx, kern_h_u, (size_t)nlay * kh * ncol, true, false)) ||
      (rc = rv.init(ctx, rhs_v_u, (size_t)kv * ncell, true, false)) || (rc = rh.init(ctx, rhs_h_u, (size_t)kh * ncell, true, false)) ||
      (rc = wv.init(ctx, w_v_u, (size_t)kv * ncell, true, false)) || (rc = wh.init(ctx, w_h_u, (size_t)kh * ncell, true, false)) ||
      (rc = d0.init(ctx, d0_u, (size_t)nlay * ncell, true, false)) || (rc = x.init(ctx, x_u, (size_t)2 * nlay * ncell, false, true)))
    return rc;
  void *pe, *pp = nullptr, *ps = nullptr;
  if ((rc = dz_scratch(ctx, "colr.empty", sizeof(int), &pe))) return rc;
  if (stats && ((rc = dz_scratch(ctx, "colr.part", (size_t)kt * ncell * 2 * sizeof(double), &pp)) ||
                (rc = dz_scratch(ctx, "colr.stats", (size_t)kt * 2 * sizeof(float), &ps))))
    return rc;
  DZ_HIP(hipMemsetAsync(pe, 0, sizeof(int), ctx->stream));
  const size_t lds = cr_lds_bytes(nlay, kt);      // more than the 64 KiB a kernel gets unasked from n = 50 or so
  DZ_HIP(hipFuncSetAttribute((const void *)k_column_lsq_radial, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const double s2 = (double)smooth * (double)smooth, d2 = (double)damp * (double)damp, m2 = (double)couple * (double)couple;
  {
    DzTimer t(ctx, "column_lsq_radial");
    hipLaunchKernelGGL(k_column_lsq_radial, dim3((unsigned)ncell), dim3(2 * nlay <= 64 ? 64 : 128), lds, ctx->stream, nx, ny, nlay, kv, kh,
                       kvb.dev, khb.dev, rv.dev, rh.dev, wv.dev, wh.dev, d0.dev, s2, d2, m2, x.dev, (int *)pe, (double *)pp);
    DZ_HIP(hipGetLastError());
    if (stats) {                                  // per wave type: its periods' partial sums against its own weights
      if (kv && (rc = dz_column_stats(ctx, ncell, kv, kv, wv.dev, (const double *)pp, (float *)ps))) return rc;
      if (kh && (rc = dz_column_stats(ctx, ncell, kh, kh, wh.dev, (const double *)pp + (size_t)kv * ncell * 2, (float *)ps + kv * 2)))
        return rc;
    }
    t.stop();
  }
  int ne = 0;
  DZ_HIP(hipMemcpyAsync(&ne, pe, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (stats) DZ_HIP(hipMemcpyAsync(stats, ps, (size_t)kt * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = x.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_empty) *n_empty = ne;
  return 0;
}

int dazim_column_resolution_radial(dazim_ctx *ctx, int nx, int ny, int nlay, int kv, const double *kern_v_u, int kh,
                                   const double *kern_h_u, const float *w_v_u, const float *w_h_u, float smooth, float damp, float couple,
                                   float *std_u, float *cov_vh_u, float *rdiag_u, float *rsum_u, float *cross_u, float *trace_u,
                                   float *rows_u, int *n_empty, int *n_failed) {
  if (!ctx) return DAZIM_E_BAD_ARG;
  int rc;
  if ((rc = cr_check(ctx, "dazim_column_resolution_radial", nx, ny, nlay, kv, kern_v_u, kh, kern_h_u, smooth, damp, couple))) return rc;
  if (!std_u || !cov_vh_u || !rdiag_u || !rsum_u || !cross_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_column_resolution_radial: an output among std, cov_vh, rdiag, rsum, cross is missing");
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (nx - 2) * (ny - 2), kt = kv + kh;
  const size_t ncol = (size_t)nx * ny, no = (size_t)2 * nlay * ncell;
  DzBuf<double> kvb, khb;
  DzBuf<float> wv, wh, sp, cv, rd, rs, cr, tr, rw;
  if ((rc = kvb.init(ctx, kern_v_u, (size_t)nlay * kv * ncol, true, false)) || (rc = khb.init(ctx, kern_h_u, (size_t)nlay * kh * ncol, true, false)) ||
      (rc = wv.init(ctx, w_v_u, (size_t)kv * ncell, true, false)) || (rc = wh.init(ctx, w_h_u, (size_t)kh * ncell, true, false)) ||
      (rc = sp.init(ctx, std_u, no, false, true)) || (rc = cv.init(ctx, cov_vh_u, no / 2, false, true)) ||
      (rc = rd.init(ctx, rdiag_u, no, false, true)) || (rc = rs.init(ctx, rsum_u, no, false, true)) ||
      (rc = cr.init(ctx, cross_u, no, false, true)) || (rc = tr.init(ctx, trace_u, (size_t)2 * ncell, false, true)) ||
      (rc = rw.init(ctx, rows_u, no * 2 * nlay, false, true)))
    return rc;
  void *pc;
  if ((rc = dz_scratch(ctx, "colr.res_cnt", 2 * sizeof(int), &pc))) return rc;
  DZ_HIP(hipMemsetAsync(pc, 0, 2 * sizeof(int), ctx->stream));
  const size_t lds = cr_lds_bytes(nlay, kt);
  DZ_HIP(hipFuncSetAttribute((const void *)k_column_res_radial, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const double s2 = (double)smooth * (double)smooth, d2 = (double)damp * (double)damp, m2 = (double)couple * (double)couple;
  {
    DzTimer t(ctx, "column_resolution_radial");
    hipLaunchKernelGGL(k_column_res_radial, dim3((unsigned)ncell), dim3(2 * nlay <= 64 ? 64 : 128), lds, ctx->stream, nx, ny, nlay, kv, kh,
                       kvb.dev, khb.dev, wv.dev, wh.dev, s2, d2, m2, sp.dev, cv.dev, rd.dev, rs.dev, cr.dev, tr.dev, rw.dev, (int *)pc);
    DZ_HIP(hipGetLastError());
    t.stop();
  }
  int cnt[2] = {0, 0};
  DZ_HIP(hipMemcpyAsync(cnt, pc, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = sp.finish()) || (rc = cv.finish()) || (rc = rd.finish()) || (rc = rs.finish()) || (rc = cr.finish()) || (rc = tr.finish()) ||
      (rc = rw.finish()))
    return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_empty) *n_empty = cnt[0];
  if (n_failed) *n_failed = cnt[1];
  return 0;
}

}  // extern "C"
