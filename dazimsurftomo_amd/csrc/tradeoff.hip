// tradeoff.hip -- dazim_model_tradeoff and dazim_map_tradeoff: a sweep over regularisation strengths of a linearised step, on the
// exact fp64 dense normal matrix of dazim_model_posterior (the direct 3-D inversion, DESIGN.md section 16: one block of
// n = nblk (nx-2)(ny-2)(nz-1) unknowns) and of dazim_map_posterior (the per-period maps, section 12.2: block diagonal by period, a
// block of n_g = nblk ncell unknowns per period).  One sweep (mt_sweep_block) serves both; a block is described to it and to its
// kernels by a view, MtModel or MtPeriod, that answers what differs: where a block's rows are, how a stored column maps to a local
// index and to a block, and how its regularisation rows and its right-hand side are gathered.  Per block:
//   once     D = sum over the data rows of r^T r (model: k_mt_gram_data, mo_accum_row on the transpose entries before regstart[a];
//            maps: k_mp_gram on the period's data rows with d^2 = 0), mirrored to both triangles; g = sum over the data rows of r^T b_r
//   point k  combine   W = D + sum_b scale[k][b]^2 R_b + damp[k]^2 I: D's row, then the regularisation rows that hold a, ascending
//            factor    dz_mp_factor (map_post_dense.hip) on W; D is never factored
//            solve     R y = g, R^T x = y: blocked by panels of MP_NB, diagonal block in one workgroup, the update over the chip
//            sums      log det, |G x - b|^2, |L_b x|^2 per block, |x|^2
//            inverse   (want_dof) dz_mp_inverse_c, then sum_c C_ac D_ac per row and the rows of a block
//            evidence  (want_evidence) W = P_k alone, factored again for log det P_k
// fp64, every sum in a fixed order that depends on the problem alone, no floating-point atomics; the dependencies between the steps
// are launch order on the context's stream.  The n x n matrices are allocated for the call and released on every way out.
#include <algorithm>
#include <cmath>
#include <vector>

#include "map_post_internal.h"

namespace {

constexpr int MT_RG = 16;    // rows per wavefront in the row sums
constexpr int MT_TR = 32;    // tile of the mirror pass

struct MtScale {
  double s2[3];
};

// ---- the two views of a block -------------------------------------------------------------------------------------------------------
// The 3-D model: the matrix is the block, a stored column is the local index, the data rows are 0 .. m_data and the regularisation
// rows follow them; both are reached per unknown through the transpose, split at regstart[a].
struct MtModel {
  typedef int64_t Idx;   // (a row's number in its part)
  int n, maxvp;
  int64_t m_data, mreg;
  const int64_t *colptr, *regstart;
  const int *row;
  const float *tval;
  const int64_t *rowptr;
  const int *col;
  const float *val;
  template <bool REG>
  __host__ __device__ __forceinline__ Idx nrows() const { return REG ? mreg : m_data; }
  template <bool REG>
  __device__ __forceinline__ int64_t rowof(Idx i) const { return REG ? m_data + i : i; }
  __device__ __forceinline__ int local(int c) const { return c; }
  __device__ __forceinline__ int block(int c) const { return c / maxvp; }
  __device__ __forceinline__ size_t dm(int a) const { return (size_t)a; }
  // Wa[c] += s2[block of a] (v_a r_c) over the regularisation rows of column a in the transpose, ascending
  __device__ __forceinline__ void add_reg(int a, int t, const MtScale &sc, double *Wa) const {
    mo_accum_row<true>(a, t, n, regstart[a], colptr[a + 1], row, tval, rowptr, col, val, sc.s2[a / maxvp], Wa);
  }
  // g[a] = sum over the data rows r of column a in the transpose of v_a b_r: lane t takes the entries t, t + 64, ..., then the butterfly
  __device__ __forceinline__ double rhs(int a, int t, const float *b) const {
    double s = 0.0;
    for (int64_t p = colptr[a] + t; p < regstart[a]; p += 64) s += (double)tval[p] * (double)b[row[p]];
    return wave_sum(s);
  }
};

// Period p of the maps: local index a = blk ncell + cell of column blk kn + p ncell + cell; the period's data rows and regularisation
// rows are two lists, ascending, and the rows that hold a are found among them (mp_rows_with).
struct MtPeriod {
  typedef int Idx;
  int n, ncell, kn, p, ndat, nreg;
  const int *ldat, *lreg, *span;
  const int64_t *rowptr;
  const int *col;
  const float *val;
  template <bool REG>
  __host__ __device__ __forceinline__ Idx nrows() const { return REG ? nreg : ndat; }
  template <bool REG>
  __device__ __forceinline__ int rowof(Idx i) const { return REG ? lreg[i] : ldat[i]; }
  __device__ __forceinline__ int local(int c) const { return mp_local(c, kn, ncell); }
  __device__ __forceinline__ int block(int c) const { return c / kn; }
  __device__ __forceinline__ size_t dm(int a) const { return (size_t)(a / ncell) * kn + (size_t)p * ncell + a % ncell; }
  // Wa[c] += s2[block of a] (r_a r_c) over the period's regularisation rows that hold a, in the order of the list
  __device__ __forceinline__ void add_reg(int a, int t, const MtScale &sc, double *Wa) const {
    mp_accum_rows<true>(a, t, ncell, kn, p, nreg, lreg, span, rowptr, col, val, sc.s2[a / ncell], Wa);
  }
  // g[a] = sum over the period's data rows r that hold column a, in the order of the list, of r_a b_r; every lane carries the same sum
  __device__ __forceinline__ double rhs(int a, int t, const float *b) const {
    double s = 0.0;
    mp_rows_with(a, t, ncell, kn, p, ndat, ldat, span, rowptr, col, val, [&s, b](long long, long long, double v, int r) { s += v * (double)b[r]; });
    return s;
  }
};

// bad |= 1 when a regularisation row has entries in two blocks of blkw columns (its columns ascend: the first and the last decide)
__global__ __launch_bounds__(MP_TB) void k_mt_span(int64_t m_data, int64_t mreg, int blkw, const int64_t *rowptr, const int *col, int *bad) {
  const int64_t l = (int64_t)blockIdx.x * MP_TB + threadIdx.x;
  if (l >= mreg) return;
  const int64_t b = rowptr[m_data + l], e = rowptr[m_data + l + 1];
  if (e > b && col[b] / blkw != col[e - 1] / blkw) atomicOr(bad, 1);
}

// row a of the model's D, c <= a: the data rows of column a in the transpose, ascending -- the first part of k_mo_gram's sum
__global__ __launch_bounds__(64) void k_mt_gram_data(int n, const int64_t *colptr, const int64_t *regstart, const int *row, const float *tval,
                                                     const int64_t *rowptr, const int *col, const float *val, double *D) {
  const int a = blockIdx.x, t = threadIdx.x;
  double *Da = D + (size_t)a * n;
  for (int c = t; c < n; c += 64) Da[c] = 0.0;
  __syncthreads();
  mo_accum_row<false>(a, t, n, colptr[a], regstart[a], row, tval, rowptr, col, val, 1.0, Da);
}

// D[c][a] = D[a][c] for c < a, tile by tile through LDS (the dot of C with D reads whole rows)
__global__ __launch_bounds__(MP_TB) void k_mt_mirror(int n, double *D) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ double T[MT_TR][MT_TR + 1];
  const int a0 = blockIdx.y * MT_TR, c0 = blockIdx.x * MT_TR, tj = threadIdx.x % MT_TR, ti0 = threadIdx.x / MT_TR;
  for (int ti = ti0; ti < MT_TR; ti += MP_TB / MT_TR) {
    const int a = a0 + ti, c = c0 + tj;
    T[ti][tj] = (a < n && c < a) ? D[(size_t)a * n + c] : 0.0;
  }
  __syncthreads();
  for (int ti = ti0; ti < MT_TR; ti += MP_TB / MT_TR) {
    const int c = c0 + ti, a = a0 + tj;
    if (a < n && c < a) D[(size_t)c * n + a] = T[tj][ti];
  }
}

// row a of the work matrix, c <= a: src's row (D; nullptr: zero, for P_k alone), then the view's regularisation rows that hold a,
// ascending, each product times the squared scale of a's block, then damp^2 on the diagonal.  At scale 1 these are the numbers of
// the posterior's Gram pass (k_mo_gram, k_mp_gram), added in its order.
template <class V>
__global__ __launch_bounds__(64) void k_mt_combine(V v, const double *src, MtScale sc, double d2, double *W) {
  const int a = blockIdx.x, t = threadIdx.x;
  double *Wa = W + (size_t)a * v.n;
  const double *Sa = src ? src + (size_t)a * v.n : nullptr;
  for (int c = t; c <= a; c += 64) Wa[c] = Sa ? Sa[c] : 0.0;
  __syncthreads();
  v.add_reg(a, t, sc, Wa);
  if (t == 0) Wa[a] += d2;
}

// g[a] = sum over the view's data rows of r_a b_r in the view's own order: one wavefront per a
template <class V>
__global__ __launch_bounds__(64) void k_mt_rhs(V v, const float *b, double *g) {
  const int a = blockIdx.x;
  const double s = v.rhs(a, threadIdx.x, b);
  if (threadIdx.x == 0) g[a] = s;
}

// ---- the triangular solves, one right-hand side, panel width MP_NB ------------------------------------------------------------------
// diagonal block [k0, k0 + nb) in one workgroup.  Forward: R y = s column by column, y_c = s_c / R_cc, then s_t -= R_tc y_c for t > c.
// TRANS: R^T x = s from the last column, x_c = s_c / R_cc, then s_t -= R_ct x_c for t < c.
template <bool TRANS>
__global__ __launch_bounds__(64) void k_mt_trsv_diag(int ng, int k0, int nb, const double *R, double *y) {
  __shared__ double S[MP_NB][MP_NB + 1], s[MP_NB];
  const int t = threadIdx.x;
  for (int q = t; q < nb * nb; q += 64) {
    const int i = q / nb, j = q - i * nb;
    if (j <= i) S[i][j] = R[(size_t)(k0 + i) * ng + k0 + j];
  }
  if (t < nb) s[t] = y[k0 + t];
  __syncthreads();
  for (int cc = 0; cc < nb; cc++) {
    const int c = TRANS ? nb - 1 - cc : cc;
    if (t == c) s[c] /= S[c][c];
    __syncthreads();
    if (TRANS) {
      if (t < c) s[t] -= S[c][t] * s[c];
    } else {
      if (t > c && t < nb) s[t] -= S[t][c] * s[c];
    }
    __syncthreads();
  }
  if (t < nb) y[k0 + t] = s[t];
}

// forward update: y_i -= sum_j R[i][k0 + j] y[k0 + j] for the rows i behind the panel; 32 lanes read a row's 32 contiguous entries,
// the products are summed by the butterfly of the half wavefront
__global__ __launch_bounds__(MP_TB) void k_mt_fwd_upd(int ng, int k0, int nb, const double *R, double *y) {
  const int j = threadIdx.x & 31;
  const int i = k0 + nb + blockIdx.x * (MP_TB / 32) + (threadIdx.x >> 5);
  double v = (i < ng && j < nb) ? R[(size_t)i * ng + k0 + j] * y[k0 + j] : 0.0;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (i < ng && j == 0) y[i] -= v;
}

// transposed update: y_i -= R[k0 + j][i] x[k0 + j] for j ascending in the panel, for the unknowns i before the panel; thread i reads
// row k0 + j of R along i
__global__ __launch_bounds__(MP_TB) void k_mt_bwd_upd(int ng, int k0, int nb, const double *R, double *y) {
  __shared__ double xs[MP_NB];
  if (threadIdx.x < nb) xs[threadIdx.x] = y[k0 + threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * MP_TB + threadIdx.x;
  if (i >= k0) return;
  double acc = y[i];
  for (int j = 0; j < nb; j++) acc -= R[(size_t)(k0 + j) * ng + i] * xs[j];
  y[i] = acc;
}

// ---- fixed-order sums ------------------------------------------------------------------------------------------------------------------
// wavefront w takes the rows w MT_RG .. of the view's data part or regularisation part: t = sum_q val_q x[local col_q] (lane l the
// entries l, l + 64, ...; butterfly), minus b_r for the data rows; t^2 goes to the slot of the row's block (data rows: slot 0), in
// the order of the part.  part [groups][3].
template <class V, bool REG>
__global__ __launch_bounds__(MP_TB) void k_mt_rows(V v, const double *x, const float *b, double *part) {
  typedef typename V::Idx Idx;
  const int lane = threadIdx.x & 63;
  const Idx nrows = v.template nrows<REG>(), g = (Idx)blockIdx.x * (MP_TB / 64) + (threadIdx.x >> 6), ngroup = (nrows + MT_RG - 1) / MT_RG;
  if (g >= ngroup) return;
  double acc[3] = {0.0, 0.0, 0.0};
  const Idx le = (g + 1) * MT_RG < nrows ? (g + 1) * MT_RG : nrows;
  for (Idx l = g * MT_RG; l < le; l++) {
    const auto r = v.template rowof<REG>(l);
    const int64_t qb = v.rowptr[r], qe = v.rowptr[r + 1];
    double s = 0.0;
    for (int64_t q = qb + lane; q < qe; q += 64) s += (double)v.val[q] * x[v.local(v.col[q])];
    s = wave_sum(s);
    if (REG) {
      if (qe > qb) acc[v.block(v.col[qb])] += s * s;
    } else {
      s -= (double)b[r];
      acc[0] += s * s;
    }
  }
  if (lane == 0)
    for (int k = 0; k < 3; k++) part[(size_t)g * 3 + k] = acc[k];
}

// out[j] = sum_i src[j step + i stride], i < count: 256 strided partial sums, combined in a fixed tree (workgroup j)
__global__ __launch_bounds__(MP_TB) void k_mt_sum(int64_t count, int stride, int64_t step, const double *src, double *out) {
  __shared__ double red[MP_TB / 64];
  const double *p = src + (size_t)blockIdx.x * step;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += MP_TB) s += p[i * stride];
  s = mp_block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// workgroup 0: *ld = 2 sum_i log R_ii; workgroup 1 (when launched): *xn = sum_i x_i^2
__global__ __launch_bounds__(MP_TB) void k_mt_logdet_norm(int n, const double *R, const double *x, double *ld, double *xn) {
  __shared__ double red[MP_TB / 64];
  double s = 0.0;
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < n; i += MP_TB) s += log(R[(size_t)i * n + i]);
  } else {
    for (int i = threadIdx.x; i < n; i += MP_TB) s += x[i] * x[i];
  }
  s = mp_block_sum(s, red);
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) *ld = 2.0 * s;
    else *xn = s;
  }
}

// rowdot[a] = sum_c C_ac D_ac (both rows contiguous; D holds both triangles)
__global__ __launch_bounds__(MP_TB) void k_mt_rowdot(int n, const double *Cm, const double *D, double *rowdot) {
  __shared__ double red[MP_TB / 64];
  const size_t o = (size_t)blockIdx.x * n;
  double s = 0.0;
  for (int c = threadIdx.x; c < n; c += MP_TB) s += Cm[o + c] * D[o + c];
  s = mp_block_sum(s, red);
  if (threadIdx.x == 0) rowdot[blockIdx.x] = s;
}

struct MtOut {
  double *chi2, *reg2, *xnorm2, *logdet_a, *logdet_p, *dof, *gcv, *logev;
};
enum { MT_CHI2 = 0, MT_REG2 = 1, MT_XN = 4, MT_LDA = 5, MT_LDP = 6, MT_DOF = 7, MT_NSC = 10 };

// the outputs of one point of one block, output slot k, from its sums sc[MT_NSC] and its m_data data rows; flag[0]: A_k could not be
// factored (every output NaN), flag[1]: P_k could not
__global__ void k_mt_final(int k, int nblk, int64_t m_data, MtScale s, double d2, int want_dof, int want_ev, const int *flag, const double *sc,
                           MtOut o) {
  const double nan = __builtin_nan("");
  const bool failed = flag[0] != 0;
  double J = d2 * sc[MT_XN], dofs = 0.0;
  for (int b = 0; b < nblk; b++) {
    J += s.s2[b] * sc[MT_REG2 + b];
    dofs += sc[MT_DOF + b];
    o.reg2[k * nblk + b] = failed ? nan : sc[MT_REG2 + b];
    if (want_dof && o.dof) o.dof[k * nblk + b] = failed ? nan : sc[MT_DOF + b];
  }
  o.chi2[k] = failed ? nan : sc[MT_CHI2];
  o.xnorm2[k] = failed ? nan : sc[MT_XN];
  o.logdet_a[k] = failed ? nan : sc[MT_LDA];
  if (want_dof && o.gcv) {
    const double den = (double)m_data - dofs;
    o.gcv[k] = failed ? nan : (double)m_data * sc[MT_CHI2] / (den * den);
  }
  if (want_ev) {
    const double ldp = (failed || flag[1] != 0) ? nan : sc[MT_LDP];
    if (o.logdet_p) o.logdet_p[k] = ldp;
    if (o.logev) o.logev[k] = failed ? nan : -0.5 * (sc[MT_CHI2] + J) + 0.5 * ldp - 0.5 * sc[MT_LDA] - 0.5 * (double)m_data * log(6.283185307179586476925);
  }
}

// the block's solution, rounded once, into the layout of dm
template <class V>
__global__ __launch_bounds__(MP_TB) void k_mt_xout(V v, const double *x, const int *flag, float *out) {
  const int a = blockIdx.x * MP_TB + threadIdx.x;
  if (a < v.n) out[v.dm(a)] = *flag ? nanf("") : (float)x[a];
}

// ---- the launches of one right-hand side on the factor R (lower triangle of Rd [n][n]), on the context's stream ----------------------
// y := R^-T R^-1 y by panels of MP_NB
int mt_solve(dazim_ctx *ctx, int n, const double *Rd, double *y) {
  for (int k0 = 0; k0 < n; k0 += MP_NB) {
    const int nb = std::min(MP_NB, n - k0), rest = n - k0 - nb;
    hipLaunchKernelGGL(k_mt_trsv_diag<false>, dim3(1), dim3(64), 0, ctx->stream, n, k0, nb, Rd, y);
    if (rest > 0)
      hipLaunchKernelGGL(k_mt_fwd_upd, dim3((unsigned)((rest + MP_TB / 32 - 1) / (MP_TB / 32))), dim3(MP_TB), 0, ctx->stream, n, k0, nb, Rd, y);
  }
  for (int k0 = ((n - 1) / MP_NB) * MP_NB; k0 >= 0; k0 -= MP_NB) {
    const int nb = std::min(MP_NB, n - k0);
    hipLaunchKernelGGL(k_mt_trsv_diag<true>, dim3(1), dim3(64), 0, ctx->stream, n, k0, nb, Rd, y);
    if (k0 > 0) hipLaunchKernelGGL(k_mt_bwd_upd, dim3((unsigned)((k0 + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, n, k0, nb, Rd, y);
  }
  DZ_HIP(hipGetLastError());
  return 0;
}

// *ld = 2 sum_i log R_ii and, with x, *xn = sum_i x_i^2
int mt_logdet_norm(dazim_ctx *ctx, int n, const double *Rd, const double *x, double *ld, double *xn) {
  hipLaunchKernelGGL(k_mt_logdet_norm, dim3(x ? 2 : 1), dim3(MP_TB), 0, ctx->stream, n, Rd, x, ld, xn);
  DZ_HIP(hipGetLastError());
  return 0;
}

int mt_mirror(dazim_ctx *ctx, int n, double *D) {
  const unsigned ntr = (unsigned)((n + MT_TR - 1) / MT_TR);
  hipLaunchKernelGGL(k_mt_mirror, dim3(ntr, ntr), dim3(MP_TB), 0, ctx->stream, n, D);
  DZ_HIP(hipGetLastError());
  return 0;
}

// out[j] = sum_{i < count} src[j step + i stride] for j < nout
int mt_sum(dazim_ctx *ctx, int nout, int64_t count, int stride, int64_t step, const double *src, double *out) {
  hipLaunchKernelGGL(k_mt_sum, dim3((unsigned)nout), dim3(MP_TB), 0, ctx->stream, count, stride, step, src, out);
  DZ_HIP(hipGetLastError());
  return 0;
}

// ---- the sweep of one block ------------------------------------------------------------------------------------------------------------
// What the blocks of one call share: the K points, the work space, the outputs, and the seconds of the four parts.
struct MtSweep {
  dazim_ctx *ctx;
  const char *lapname;
  bool mfma;
  int K, nblk, want_dof, want_ev;
  const float *scale, *damp;   // [K][nblk], [K] (host)
  double *D, *W, *C;           // [n][n]; C only with want_dof
  double *g, *y, *part, *rowdot, *sc;
  int *flags;                  // two per output slot: A_k, P_k could not be factored
  MtOut out;
  float *x;                    // [K][xstride] in the layout of dm, or nullptr
  size_t xstride;
  double sec[4] = {0, 0, 0, 0};   // gram, factor, solve, inverse
};

// g[a] of the view's block into w.g
template <class V>
int mt_rhs(MtSweep &w, const V &v, const float *b) {
  dazim_ctx *ctx = w.ctx;
  hipLaunchKernelGGL(k_mt_rhs<V>, dim3((unsigned)v.n), dim3(64), 0, ctx->stream, v, b, w.g);
  DZ_HIP(hipGetLastError());
  return 0;
}

// All K points of the block that v describes, whose D and g are on the device and whose m_data data rows have the right-hand side b;
// point k writes the output slot slot(k).
template <class V, class Slot>
int mt_sweep_block(MtSweep &w, const V &v, int64_t m_data, const float *b, Slot slot) {
  dazim_ctx *ctx = w.ctx;
  const int n = v.n, nblk = w.nblk;
  const int64_t gdata = ((int64_t)v.template nrows<false>() + MT_RG - 1) / MT_RG, greg = ((int64_t)v.template nrows<true>() + MT_RG - 1) / MT_RG;
  const unsigned nvb = (unsigned)((n + MP_TB - 1) / MP_TB);
  int rc;
  for (int k = 0; k < w.K; k++) {
    MtScale s;
    for (int j = 0; j < 3; j++) s.s2[j] = j < nblk ? (double)w.scale[k * nblk + j] * (double)w.scale[k * nblk + j] : 0.0;
    const double d2 = (double)w.damp[k] * (double)w.damp[k];
    const int kp = slot(k);
    int *fl = w.flags + 2 * (size_t)kp;
    {
      DzTimer t(ctx, w.lapname);
      hipLaunchKernelGGL(k_mt_combine<V>, dim3((unsigned)n), dim3(64), 0, ctx->stream, v, (const double *)w.D, s, d2, w.W);
      DZ_HIP(hipGetLastError());
      t.lap(w.sec[1]);
    }
    if ((rc = dz_mp_factor(ctx, n, w.W, fl, w.mfma, w.lapname, w.sec + 1))) return rc;
    {
      DzTimer t(ctx, w.lapname);
      DZ_HIP(hipMemsetAsync(w.sc, 0, MT_NSC * sizeof(double), ctx->stream));
      DZ_HIP(hipMemcpyAsync(w.y, w.g, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      if ((rc = mt_solve(ctx, n, w.W, w.y)) || (rc = mt_logdet_norm(ctx, n, w.W, w.y, w.sc + MT_LDA, w.sc + MT_XN))) return rc;
      if (gdata > 0) {
        hipLaunchKernelGGL((k_mt_rows<V, false>), dim3((unsigned)((gdata + MP_TB / 64 - 1) / (MP_TB / 64))), dim3(MP_TB), 0, ctx->stream, v,
                           (const double *)w.y, b, w.part);
        if ((rc = mt_sum(ctx, 1, gdata, 3, 1, w.part, w.sc + MT_CHI2))) return rc;
      }
      if (greg > 0) {
        hipLaunchKernelGGL((k_mt_rows<V, true>), dim3((unsigned)((greg + MP_TB / 64 - 1) / (MP_TB / 64))), dim3(MP_TB), 0, ctx->stream, v,
                           (const double *)w.y, (const float *)nullptr, w.part);
        if ((rc = mt_sum(ctx, nblk, greg, 3, 1, w.part, w.sc + MT_REG2))) return rc;
      }
      if (w.x) hipLaunchKernelGGL(k_mt_xout<V>, dim3(nvb), dim3(MP_TB), 0, ctx->stream, v, (const double *)w.y, (const int *)fl, w.x + (size_t)k * w.xstride);
      DZ_HIP(hipGetLastError());
      t.lap(w.sec[2]);
    }
    if (w.want_dof) {
      double s3[3] = {0, 0, 0};
      if ((rc = dz_mp_inverse_c(ctx, n, w.W, w.C, w.mfma, w.lapname, s3))) return rc;
      DzTimer t(ctx, w.lapname);
      hipLaunchKernelGGL(k_mt_rowdot, dim3((unsigned)n), dim3(MP_TB), 0, ctx->stream, n, (const double *)w.C, (const double *)w.D, w.rowdot);
      DZ_HIP(hipGetLastError());
      if ((rc = mt_sum(ctx, nblk, n / nblk, 1, n / nblk, w.rowdot, w.sc + MT_DOF))) return rc;
      t.lap(w.sec[3]);
      w.sec[3] += s3[1] + s3[2];
    }
    if (w.want_ev) {
      {
        DzTimer t(ctx, w.lapname);
        hipLaunchKernelGGL(k_mt_combine<V>, dim3((unsigned)n), dim3(64), 0, ctx->stream, v, (const double *)nullptr, s, d2, w.W);
        DZ_HIP(hipGetLastError());
        t.lap(w.sec[1]);
      }
      if ((rc = dz_mp_factor(ctx, n, w.W, fl + 1, w.mfma, w.lapname, w.sec + 1))) return rc;
      DzTimer t(ctx, w.lapname);
      if ((rc = mt_logdet_norm(ctx, n, w.W, nullptr, w.sc + MT_LDP, nullptr))) return rc;
      t.lap(w.sec[1]);
    }
    hipLaunchKernelGGL(k_mt_final, dim3(1), dim3(1), 0, ctx->stream, kp, nblk, m_data, s, d2, w.want_dof, w.want_ev, (const int *)fl,
                       (const double *)w.sc, w.out);
    DZ_HIP(hipGetLastError());
  }
  return 0;
}

// ---- what the two entries ask of their arguments alike ---------------------------------------------------------------------------------
// sizes_ok, outs_ok: the entry's own grid sizes and required outputs; n_want = the unknowns its sizes give (n_what in words), at most
// n_max.  The messages carry the entry's name.
int mt_check_args(dazim_ctx *ctx, const char *name, const dazim_csr *A, bool sizes_ok, bool outs_ok, int64_t m_data, const float *b, int nblk,
                  int64_t n_want, int64_t n_max, const char *n_what, int K, const float *scale, const float *damp, int want_dof, bool dof_out,
                  int want_evidence, bool ev_out) {
  if (!ctx || !A || !sizes_ok || !scale || !damp || !outs_ok) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to %s", name);
  if (dz_is_device_ptr(scale) || dz_is_device_ptr(damp)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: scale and damp are host arrays", name);
  if (K < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: K %d < 1", name, K);
  if (!b) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: no right-hand side b", name);
  if (m_data < 0 || m_data > A->m) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: m_data %lld outside 0..%lld", name, (long long)m_data, (long long)A->m);
  if (A->n != n_want || n_want > n_max) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: n %lld is not %s = %lld", name, (long long)A->n, n_what, (long long)n_want);
  if (!want_dof && dof_out) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: dof or gcv without want_dof", name);
  if (!want_evidence && ev_out) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: logdet_p or logev without want_evidence", name);
  for (int k = 0; k < K; k++) {
    if (!(damp[k] >= 0.0f) || !std::isfinite(damp[k])) return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: damp[%d] negative or not finite", name, k);
    for (int j = 0; j < nblk; j++)
      if (!(scale[k * nblk + j] >= 0.0f) || !std::isfinite(scale[k * nblk + j]))
        return dz_fail(ctx, DAZIM_E_BAD_ARG, "%s: scale[%d][%d] negative or not finite", name, k, j);
  }
  return 0;
}

// the outputs of a call, [slots] per point-and-block array, staged where the user's arrays are on the host
struct MtBufs {
  DzBuf<float> bb, xo;
  DzBuf<double> chi, reg, xn, lda, ldp, dof, gcv, lev;
  int init(dazim_ctx *ctx, const float *b_u, size_t m_data, float *x_u, size_t nx, size_t slots, int nblk, double *chi2_u, double *reg2_u,
           double *xnorm2_u, double *logdet_a_u, double *logdet_p_u, double *dof_u, double *gcv_u, double *logev_u) {
    int rc;
    if ((rc = bb.init(ctx, b_u, m_data, true, false)) || (rc = xo.init(ctx, x_u, x_u ? nx : 0, false, true)) ||
        (rc = chi.init(ctx, chi2_u, slots, false, true)) || (rc = reg.init(ctx, reg2_u, slots * nblk, false, true)) ||
        (rc = xn.init(ctx, xnorm2_u, slots, false, true)) || (rc = lda.init(ctx, logdet_a_u, slots, false, true)) ||
        (rc = ldp.init(ctx, logdet_p_u, logdet_p_u ? slots : 0, false, true)) || (rc = dof.init(ctx, dof_u, dof_u ? slots * nblk : 0, false, true)) ||
        (rc = gcv.init(ctx, gcv_u, gcv_u ? slots : 0, false, true)) || (rc = lev.init(ctx, logev_u, logev_u ? slots : 0, false, true)))
      return rc;
    return 0;
  }
  MtOut out() const { return {chi.dev, reg.dev, xn.dev, lda.dev, ldp.dev, dof.dev, gcv.dev, lev.dev}; }
  int finish() {
    int rc;
    if ((rc = xo.finish()) || (rc = chi.finish()) || (rc = reg.finish()) || (rc = xn.finish()) || (rc = lda.finish()) || (rc = ldp.finish()) ||
        (rc = dof.finish()) || (rc = gcv.finish()) || (rc = lev.finish()))
      return rc;
    return 0;
  }
};

}  // namespace

extern "C" int dazim_model_tradeoff(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, const float *b_u, int nx, int ny, int nz, int joint, int K,
                                    const float *scale, const float *damp, int want_dof, int want_evidence, double *chi2_u, double *reg2_u,
                                    double *xnorm2_u, double *logdet_a_u, double *logdet_p_u, double *dof_u, double *gcv_u, double *logev_u,
                                    float *x_u, int *n_failed) {
  const int nblk = joint ? 3 : 1, nlay = nz - 1;
  const int64_t ncell64 = (int64_t)(nx - 2) * (ny - 2), n64 = nblk * ncell64 * nlay;
  int rc;
  if ((rc = mt_check_args(ctx, "dazim_model_tradeoff", A, nx >= 3 && ny >= 3 && nz >= 2, chi2_u && reg2_u && xnorm2_u && logdet_a_u, m_data, b_u, nblk,
                          n64, (int64_t)1 << 30, "nblk * (nx-2)(ny-2)(nz-1)", K, scale, damp, want_dof, dof_u || gcv_u, want_evidence,
                          logdet_p_u || logev_u)))
    return rc;
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_fmm_finish(ctx)) || (rc = dz_join_aux(ctx))) return rc;
  const int ncell = (int)ncell64, n = (int)n64, maxvp = ncell * nlay;
  const int64_t m = A->m, mreg = m - m_data;
  // ---- the workspace: refused before the first launch when the card cannot hold it ----
  const size_t bA = (size_t)n * n * 8, bC = want_dof ? (size_t)n * (n > MP_NB ? n : MP_NB) * 8 : 0;
  const size_t bTr = A->colptr ? 0 : (size_t)(n + 1) * 8 + (size_t)(A->nnz > 0 ? A->nnz : 1) * 12 * 3;   // (the transpose and its sort)
  if ((rc = dz_need_device_bytes(ctx, 2 * bA + bC + bTr + ((size_t)64 << 20), "dazim_model_tradeoff", (long long)n64, "unknowns"))) return rc;
  if (!A->colptr && (rc = dz_build_transpose(ctx, const_cast<dazim_csr *>(A)))) return rc;
  DzOwned big;
  DZ_HIP(dz_malloc_retry(ctx, &big.p[0], bA));
  DZ_HIP(dz_malloc_retry(ctx, &big.p[1], bA));
  if (want_dof) DZ_HIP(dz_malloc_retry(ctx, &big.p[2], bC));
  MtSweep w = {ctx, "model_trade.lap", dz_opt(ctx, "map_post.mfma", 1) != 0, K, nblk, want_dof, want_evidence, scale, damp,
               (double *)big.p[0], (double *)big.p[1], (double *)big.p[2]};
  const int64_t gdata = (m_data + MT_RG - 1) / MT_RG, greg = (mreg + MT_RG - 1) / MT_RG;
  int64_t *regstart;
  if ((rc = dz_scratch(ctx, "motrade.g", (size_t)n, &w.g)) || (rc = dz_scratch(ctx, "motrade.y", (size_t)n, &w.y)) ||
      (rc = dz_scratch(ctx, "motrade.part", (size_t)std::max<int64_t>(std::max(gdata, greg), 1) * 3, &w.part)) ||
      (rc = dz_scratch(ctx, "motrade.rowdot", (size_t)n, &w.rowdot)) || (rc = dz_scratch(ctx, "motrade.sc", (size_t)MT_NSC, &w.sc)) ||
      (rc = dz_scratch(ctx, "motrade.reg", (size_t)n, &regstart)) || (rc = dz_scratch(ctx, "motrade.flags", (size_t)(2 * K + 2), &w.flags)))
    return rc;
  MtBufs u;
  const size_t kk = (size_t)K;
  if ((rc = u.init(ctx, b_u, (size_t)m_data, x_u, kk * n, kk, nblk, chi2_u, reg2_u, xnorm2_u, logdet_a_u, logdet_p_u, dof_u, gcv_u, logev_u))) return rc;
  w.out = u.out();
  w.x = u.xo.dev;
  w.xstride = (size_t)n;
  std::vector<int> hflag((size_t)(2 * K + 2), 0);
  int *bad = w.flags + 2 * K;
  DZ_HIP(hipMemsetAsync(w.flags, 0, (size_t)(2 * K + 2) * sizeof(int), ctx->stream));
  if ((rc = dz_mo_check_rows(ctx, A, n, bad))) return rc;
  if (mreg > 0)
    hipLaunchKernelGGL(k_mt_span, dim3((unsigned)((mreg + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, m_data, mreg, maxvp, A->rowptr, A->col, bad + 1);
  DZ_HIP(hipGetLastError());
  DZ_HIP(hipMemcpyAsync(hflag.data() + 2 * K, bad, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (hflag[2 * K]) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: a row's columns do not ascend strictly inside 0..n-1");
  if (hflag[2 * K + 1]) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: a regularisation row spans two blocks");
  const MtModel v = {n, maxvp, m_data, mreg, A->colptr, regstart, A->row, A->tval, A->rowptr, A->col, A->val};
  {
    DzTimer t(ctx, w.lapname);
    if ((rc = dz_mo_regstart(ctx, A, n, m_data, regstart))) return rc;
    hipLaunchKernelGGL(k_mt_gram_data, dim3((unsigned)n), dim3(64), 0, ctx->stream, n, A->colptr, regstart, A->row, A->tval, A->rowptr, A->col, A->val, w.D);
    if ((rc = mt_mirror(ctx, n, w.D)) || (rc = mt_rhs(w, v, u.bb.dev))) return rc;
    DZ_HIP(hipMemsetAsync(w.W, 0, bA, ctx->stream));   // (the upper triangle of the work matrix is never written or read)
    t.lap(w.sec[0]);
  }
  if ((rc = mt_sweep_block(w, v, m_data, u.bb.dev, [](int k) { return k; }))) return rc;
  DZ_HIP(hipMemcpyAsync(hflag.data(), w.flags, (size_t)(2 * K) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = u.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_failed)
    for (int k = 0; k < K; k++) n_failed[k] = hflag[2 * k] != 0;
  static const char *names[4] = {"model_trade.gram", "model_trade.factor", "model_trade.solve", "model_trade.inverse"};
  dz_publish_laps(ctx, w.lapname, names, w.sec, 4, "model_tradeoff");
  ctx->ksec["model_trade.points"] = (double)K;
  ctx->ksec["model_trade.n"] = (double)n;
  return 0;
}

extern "C" int dazim_map_tradeoff(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, const float *b_u, int nx, int ny, int kmax, int azim, int K,
                                  const float *scale, const float *damp, int want_dof, int want_evidence, int64_t *mdata_p_u, double *chi2_u,
                                  double *reg2_u, double *xnorm2_u, double *logdet_a_u, double *logdet_p_u, double *dof_u, double *gcv_u,
                                  double *logev_u, float *x_u, int *n_failed) {
  const int nblk = azim ? 3 : 1;
  const int64_t ncell64 = (int64_t)(nx - 2) * (ny - 2), ng64 = nblk * ncell64;
  int rc;
  if ((rc = mt_check_args(ctx, "dazim_map_tradeoff", A, nx >= 3 && ny >= 3 && kmax >= 1, chi2_u && reg2_u && xnorm2_u && logdet_a_u, m_data, b_u, nblk,
                          ng64 * kmax, INT64_MAX, "nblk * kmax * ncell", K, scale, damp, want_dof, dof_u || gcv_u, want_evidence,
                          logdet_p_u || logev_u)))
    return rc;
  DZ_HIP(hipSetDevice(ctx->device));
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (int)ncell64, ng = (int)ng64, kn = kmax * ncell;
  const int64_t m = A->m, mreg = m - m_data, n = A->n;
  // ---- the workspace: refused before the first launch when the card cannot hold it ----
  const size_t bA = (size_t)ng * ng * 8, bC = want_dof ? (size_t)ng * (ng > MP_NB ? ng : MP_NB) * 8 : 0;
  if ((rc = dz_need_device_bytes(ctx, 2 * bA + bC + (size_t)m * 16 + ((size_t)64 << 20), "dazim_map_tradeoff", (long long)ng64, "unknowns per period")))
    return rc;
  DzOwned big;
  DZ_HIP(dz_malloc_retry(ctx, &big.p[0], bA));
  DZ_HIP(dz_malloc_retry(ctx, &big.p[1], bA));
  if (want_dof) DZ_HIP(dz_malloc_retry(ctx, &big.p[2], bC));
  MtSweep w = {ctx, "map_trade.lap", dz_opt(ctx, "map_post.mfma", 1) != 0, K, nblk, want_dof, want_evidence, scale, damp,
               (double *)big.p[0], (double *)big.p[1], (double *)big.p[2]};
  int *per, *span, *cnt, *list;
  const size_t kk = (size_t)K * kmax;
  if ((rc = dz_scratch(ctx, "mptrade.g", (size_t)ng, &w.g)) || (rc = dz_scratch(ctx, "mptrade.y", (size_t)ng, &w.y)) ||
      (rc = dz_scratch(ctx, "mptrade.part", (size_t)(m / MT_RG + 2) * 3, &w.part)) || (rc = dz_scratch(ctx, "mptrade.rowdot", (size_t)ng, &w.rowdot)) ||
      (rc = dz_scratch(ctx, "mptrade.sc", (size_t)MT_NSC, &w.sc)) || (rc = dz_scratch(ctx, "mptrade.per", (size_t)std::max<int64_t>(m, 1), &per)) ||
      (rc = dz_scratch(ctx, "mptrade.span", (size_t)2 * std::max<int64_t>(m, 1), &span)) ||
      (rc = dz_scratch(ctx, "mptrade.list", (size_t)std::max<int64_t>(m, 1), &list)) || (rc = dz_scratch(ctx, "mptrade.cnt", (size_t)2 * kmax + 1, &cnt)) ||
      (rc = dz_scratch(ctx, "mptrade.flags", 2 * kk + 1, &w.flags)))
    return rc;
  MtBufs u;
  if ((rc = u.init(ctx, b_u, (size_t)m_data, x_u, (size_t)K * n, kk, nblk, chi2_u, reg2_u, xnorm2_u, logdet_a_u, logdet_p_u, dof_u, gcv_u, logev_u)))
    return rc;
  w.out = u.out();
  w.x = u.xo.dev;
  w.xstride = (size_t)n;
  // ---- the rows of every period, and the block of every regularisation row ----
  std::vector<int> hflag(2 * kk + 1, 0), hcnt;
  int *bad = w.flags + 2 * kk;
  DZ_HIP(hipMemsetAsync(w.flags, 0, (2 * kk + 1) * sizeof(int), ctx->stream));
  if (mreg > 0)
    hipLaunchKernelGGL(k_mt_span, dim3((unsigned)((mreg + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, m_data, mreg, kn, A->rowptr, A->col, bad);
  DZ_HIP(hipGetLastError());
  DZ_HIP(hipMemcpyAsync(hflag.data() + 2 * kk, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = dz_mp_period_rows(ctx, A, m_data, kmax, kn, ncell, per, span, cnt, list, hcnt))) return rc;   // (synchronises)
  if (hcnt[2 * kmax] & 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: a row's columns lie in two periods");
  if (hcnt[2 * kmax] & 2) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: a row's columns do not ascend strictly");
  if (hflag[2 * kk]) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_tradeoff: a regularisation row spans two blocks");
  std::vector<int64_t> hmp((size_t)kmax);
  DZ_HIP(hipMemsetAsync(w.W, 0, bA, ctx->stream));   // (the upper triangle of the work matrix is never written or read)
  int off = 0, grams = 0;
  for (int p = 0; p < kmax; p++) {
    const int nrow = hcnt[2 * p], ndat = hcnt[2 * p + 1];
    const int *lp = list + off;
    off += nrow;
    hmp[p] = ndat;
    const MtPeriod v = {ng, ncell, kn, p, ndat, nrow - ndat, lp, lp + ndat, span, A->rowptr, A->col, A->val};
    {
      DzTimer t(ctx, w.lapname);
      if ((rc = dz_mp_gram(ctx, ng, ncell, kn, p, ndat, lp, span, A, 0.0, w.D)) || (rc = mt_mirror(ctx, ng, w.D))) return rc;
      grams++;
      if ((rc = mt_rhs(w, v, u.bb.dev))) return rc;
      t.lap(w.sec[0]);
    }
    if ((rc = mt_sweep_block(w, v, (int64_t)ndat, u.bb.dev, [=](int k) { return k * kmax + p; }))) return rc;
  }
  const bool mp_dev = mdata_p_u && dz_is_device_ptr(mdata_p_u);
  if (mp_dev) DZ_HIP(hipMemcpyAsync(mdata_p_u, hmp.data(), (size_t)kmax * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync(hflag.data(), w.flags, 2 * kk * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = u.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (mdata_p_u && !mp_dev)
    for (int p = 0; p < kmax; p++) mdata_p_u[p] = hmp[p];
  if (n_failed)
    for (size_t i = 0; i < kk; i++) n_failed[i] = hflag[2 * i] != 0;
  static const char *names[4] = {"map_trade.gram", "map_trade.factor", "map_trade.solve", "map_trade.inverse"};
  dz_publish_laps(ctx, w.lapname, names, w.sec, 4, "map_tradeoff");
  ctx->ksec["map_trade.points"] = (double)K;
  ctx->ksec["map_trade.ng"] = (double)ng;
  ctx->ksec["map_trade.grams"] = (double)grams;
  return 0;
}

// The three picks of a sweep (host only): the point of smallest finite gcv, of largest finite logev, and the corner of the L-curve, the
// interior point of largest Menger curvature 2 |(q - p) x (r - q)| / (|pq| |qr| |rp|) of the polyline (log chi2, log reg2sum) through
// the points where both are finite, in the order given.  -1 where there is no finite value, or fewer than three finite points.
extern "C" int dazim_tradeoff_pick(int K, const double *chi2, const double *reg2sum, const double *gcv, const double *logev, int *corner, int *igcv,
                                   int *iev) {
  int ig = -1, ie = -1, ic = -1;
  for (int k = 0; k < K; k++) {
    if (gcv && std::isfinite(gcv[k]) && (ig < 0 || gcv[k] < gcv[ig])) ig = k;
    if (logev && std::isfinite(logev[k]) && (ie < 0 || logev[k] > logev[ie])) ie = k;
  }
  if (chi2 && reg2sum) {
    std::vector<int> idx;
    std::vector<double> px, py;
    for (int k = 0; k < K; k++) {
      const double u = std::log(chi2[k]), v = std::log(reg2sum[k]);
      if (std::isfinite(u) && std::isfinite(v)) {
        idx.push_back(k);
        px.push_back(u);
        py.push_back(v);
      }
    }
    double best = -1.0;
    for (size_t i = 1; i + 1 < idx.size(); i++) {
      const double ax = px[i] - px[i - 1], ay = py[i] - py[i - 1], bx = px[i + 1] - px[i], by = py[i + 1] - py[i];
      const double cx = px[i + 1] - px[i - 1], cy = py[i + 1] - py[i - 1];
      const double den = std::sqrt(ax * ax + ay * ay) * std::sqrt(bx * bx + by * by) * std::sqrt(cx * cx + cy * cy);
      const double curv = den > 0.0 ? 2.0 * std::fabs(ax * by - ay * bx) / den : 0.0;
      if (curv > best) {
        best = curv;
        ic = idx[i];
      }
    }
  }
  if (corner) *corner = ic;
  if (igcv) *igcv = ig;
  if (iev) *iev = ie;
  return 0;
}

// The criteria of the whole block-diagonal system from dazim_map_tradeoff's per-period arrays (host only): every total the sum over
// the periods in ascending p (reg2sum_t and dof_t over p and then blk), gcv_t = M chi2_t / (M - dof_t)^2 with M = sum_p m_p.
extern "C" int dazim_map_tradeoff_total(int K, int kmax, int nblk, const int64_t *mdata_p, const double *chi2, const double *reg2, const double *dof,
                                        const double *logev, double *chi2_t, double *reg2sum_t, double *dof_t, double *gcv_t, double *logev_t) {
  if (K < 1 || kmax < 1 || nblk < 1 || !mdata_p || !chi2 || !reg2 || !chi2_t || !reg2sum_t) return DAZIM_E_BAD_ARG;
  if ((!dof && (dof_t || gcv_t)) || (!logev && logev_t)) return DAZIM_E_BAD_ARG;
  double M = 0.0;
  for (int p = 0; p < kmax; p++) M += (double)mdata_p[p];
  for (int k = 0; k < K; k++) {
    double c = 0.0, r = 0.0, d = 0.0, e = 0.0;
    for (int p = 0; p < kmax; p++) {
      const size_t kp = (size_t)k * kmax + p;
      c += chi2[kp];
      if (logev) e += logev[kp];
      for (int b = 0; b < nblk; b++) {
        r += reg2[kp * nblk + b];
        if (dof) d += dof[kp * nblk + b];
      }
    }
    chi2_t[k] = c;
    reg2sum_t[k] = r;
    if (dof_t) dof_t[k] = d;
    if (gcv_t) gcv_t[k] = M * c / ((M - d) * (M - d));
    if (logev_t) logev_t[k] = e;
  }
  return 0;
}
