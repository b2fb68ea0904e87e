// model_tradeoff.hip -- dazim_model_tradeoff: a sweep over regularisation strengths of the direct 3-D inversion's linearised step
// (DESIGN.md section 16), on the exact fp64 dense normal matrix of dazim_model_posterior.  n = nblk (nx-2)(ny-2)(nz-1) unknowns:
//   once     D = sum over the data rows of r^T r (mo_accum_row on the transpose entries before regstart[a]), mirrored to both
//            triangles; g = sum over the data rows of r^T b_r
//   point k  combine   W = D + sum_b scale[k][b]^2 R_b + damp[k]^2 I, the regularisation entries regstart[a] .. colptr[a+1] of row a
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

// bad |= 1 when a regularisation row has entries in two blocks (its columns ascend: the first and the last decide)
__global__ __launch_bounds__(MP_TB) void k_mt_span(int64_t m_data, int64_t mreg, int maxvp, const int64_t *rowptr, const int *col, int *bad) {
  const int64_t l = (int64_t)blockIdx.x * MP_TB + threadIdx.x;
  if (l >= mreg) return;
  const int64_t b = rowptr[m_data + l], e = rowptr[m_data + l + 1];
  if (e > b && col[b] / maxvp != col[e - 1] / maxvp) atomicOr(bad, 1);
}

// row a of D, c <= a: the data rows of column a in the transpose, ascending -- the first part of k_mo_gram's sum
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

// row a of the work matrix, c <= a: src's row (D; nullptr: zero, for P_k alone), then the regularisation rows of column a in the
// transpose, ascending, each product times the squared scale of a's block, then damp^2 on the diagonal.  At scale 1 these are
// k_mo_gram's numbers, added in k_mo_gram's order.
__global__ __launch_bounds__(64) void k_mt_combine(int n, int maxvp, const int64_t *colptr, const int64_t *regstart, const int *row,
                                                   const float *tval, const int64_t *rowptr, const int *col, const float *val,
                                                   const double *src, MtScale sc, double d2, double *W) {
  const int a = blockIdx.x, t = threadIdx.x;
  double *Wa = W + (size_t)a * n;
  const double *Sa = src ? src + (size_t)a * n : nullptr;
  for (int c = t; c <= a; c += 64) Wa[c] = Sa ? Sa[c] : 0.0;
  __syncthreads();
  mo_accum_row<true>(a, t, n, regstart[a], colptr[a + 1], row, tval, rowptr, col, val, sc.s2[a / maxvp], Wa);
  if (t == 0) Wa[a] += d2;
}

// g[a] = sum over the data rows r of column a in the transpose of v_a b_r: lane t takes the entries t, t + 64, ..., then the butterfly
__global__ __launch_bounds__(64) void k_mt_rhs(const int64_t *colptr, const int64_t *regstart, const int *row, const float *tval,
                                               const float *b, double *g) {
  const int a = blockIdx.x;
  double s = 0.0;
  for (int64_t p = colptr[a] + threadIdx.x; p < regstart[a]; p += 64) s += (double)tval[p] * (double)b[row[p]];
  s = wave_sum(s);
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
// wavefront w takes the rows row0 + w MT_RG .. of the matrix: t = sum_q val_q x[col_q] (lane l the entries l, l + 64, ...; butterfly),
// minus b_r for the data rows; t^2 goes to the slot of the row's block (data rows: slot 0), rows ascending.  part [groups][3].
template <bool REG>
__global__ __launch_bounds__(MP_TB) void k_mt_rows(int64_t row0, int64_t nrows, int maxvp, const int64_t *rowptr, const int *col, const float *val,
                                                   const double *x, const float *b, double *part) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * (MP_TB / 64) + (threadIdx.x >> 6), ngroup = (nrows + MT_RG - 1) / MT_RG;
  if (g >= ngroup) return;
  double acc[3] = {0.0, 0.0, 0.0};
  const int64_t le = (g + 1) * MT_RG < nrows ? (g + 1) * MT_RG : nrows;
  for (int64_t l = g * MT_RG; l < le; l++) {
    const int64_t r = row0 + l, qb = rowptr[r], qe = rowptr[r + 1];
    double s = 0.0;
    for (int64_t q = qb + lane; q < qe; q += 64) s += (double)val[q] * x[col[q]];
    s = wave_sum(s);
    if (REG) {
      if (qe > qb) acc[col[qb] / maxvp] += s * s;
    } else {
      s -= (double)b[r];
      acc[0] += s * s;
    }
  }
  if (lane == 0)
    for (int k = 0; k < 3; k++) part[g * 3 + k] = acc[k];
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

// point k's outputs from its sums sc[MT_NSC]; flag[0]: A_k could not be factored (every output NaN), flag[1]: P_k could not
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

__global__ __launch_bounds__(MP_TB) void k_mt_xout(int n, const double *x, const int *flag, float *out) {
  const int i = blockIdx.x * MP_TB + threadIdx.x;
  if (i < n) out[i] = *flag ? nanf("") : (float)x[i];
}

struct MtBig {   // the call's own allocations: released on every way out
  void *p[3] = {nullptr, nullptr, nullptr};
  ~MtBig() {
    for (void *q : p)
      if (q) (void)hipFree(q);
  }
};

}  // namespace

// ---- what dazim_map_tradeoff (map_tradeoff.hip) shares, declared in map_post_internal.h: the launches below, in this order ----
int dz_mt_solve(dazim_ctx *ctx, int n, const double *Rd, double *y) {
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

int dz_mt_logdet_norm(dazim_ctx *ctx, int n, const double *Rd, const double *x, double *ld, double *xn) {
  hipLaunchKernelGGL(k_mt_logdet_norm, dim3(x ? 2 : 1), dim3(MP_TB), 0, ctx->stream, n, Rd, x, ld, xn);
  DZ_HIP(hipGetLastError());
  return 0;
}

int dz_mt_mirror(dazim_ctx *ctx, int n, double *D) {
  const unsigned ntr = (unsigned)((n + MT_TR - 1) / MT_TR);
  hipLaunchKernelGGL(k_mt_mirror, dim3(ntr, ntr), dim3(MP_TB), 0, ctx->stream, n, D);
  DZ_HIP(hipGetLastError());
  return 0;
}

int dz_mt_rowdot(dazim_ctx *ctx, int n, const double *Cm, const double *D, double *rowdot) {
  hipLaunchKernelGGL(k_mt_rowdot, dim3((unsigned)n), dim3(MP_TB), 0, ctx->stream, n, Cm, D, rowdot);
  DZ_HIP(hipGetLastError());
  return 0;
}

int dz_mt_sum(dazim_ctx *ctx, int nout, int64_t count, int stride, int64_t step, const double *src, double *out) {
  hipLaunchKernelGGL(k_mt_sum, dim3((unsigned)nout), dim3(MP_TB), 0, ctx->stream, count, stride, step, src, out);
  DZ_HIP(hipGetLastError());
  return 0;
}

extern "C" int dazim_model_tradeoff(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, const float *b_u, int nx, int ny, int nz, int joint, int K,
                                    const float *scale, const float *damp, int want_dof, int want_evidence, double *chi2_u, double *reg2_u,
                                    double *xnorm2_u, double *logdet_a_u, double *logdet_p_u, double *dof_u, double *gcv_u, double *logev_u,
                                    float *x_u, int *n_failed) {
  if (!ctx || !A || nx < 3 || ny < 3 || nz < 2 || !scale || !damp || !chi2_u || !reg2_u || !xnorm2_u || !logdet_a_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_model_tradeoff");
  if (dz_is_device_ptr(scale) || dz_is_device_ptr(damp)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: scale and damp are host arrays");
  if (K < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: K %d < 1", K);
  if (!b_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: no right-hand side b");
  if (m_data < 0 || m_data > A->m)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: m_data %lld outside 0..%lld", (long long)m_data, (long long)A->m);
  const int nblk = joint ? 3 : 1, nlay = nz - 1;
  const int64_t ncell64 = (int64_t)(nx - 2) * (ny - 2), n64 = nblk * ncell64 * nlay;
  if (A->n != n64 || n64 > (int64_t)1 << 30)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: n %lld is not nblk * (nx-2)(ny-2)(nz-1) = %lld", (long long)A->n, (long long)n64);
  if (!want_dof && (dof_u || gcv_u)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: dof or gcv without want_dof");
  if (!want_evidence && (logdet_p_u || logev_u)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: logdet_p or logev without want_evidence");
  for (int k = 0; k < K; k++) {
    if (!(damp[k] >= 0.0f) || !std::isfinite(damp[k])) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: damp[%d] negative or not finite", k);
    for (int b = 0; b < nblk; b++)
      if (!(scale[k * nblk + b] >= 0.0f) || !std::isfinite(scale[k * nblk + b]))
        return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: scale[%d][%d] negative or not finite", k, b);
  }
  DZ_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = dz_fmm_finish(ctx)) || (rc = dz_join_aux(ctx))) return rc;
  const int ncell = (int)ncell64, n = (int)n64, maxvp = ncell * nlay;
  const int64_t m = A->m, mreg = m - m_data;
  // ---- the workspace: refused before the first launch when the card cannot hold it ----
  const size_t bA = (size_t)n * n * 8, bC = want_dof ? (size_t)n * (n > MP_NB ? n : MP_NB) * 8 : 0;
  const size_t bTr = A->colptr ? 0 : (size_t)(n + 1) * 8 + (size_t)(A->nnz > 0 ? A->nnz : 1) * 12 * 3;   // (the transpose and its sort)
  const size_t need = 2 * bA + bC + bTr + ((size_t)64 << 20);
  size_t fre = 0, tot = 0;
  DZ_HIP(hipMemGetInfo(&fre, &tot));
  if (need > fre) {
    (void)dz_trim_caches(ctx);
    DZ_HIP(hipMemGetInfo(&fre, &tot));
  }
  if (need > fre)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: %lld unknowns need %.1f GiB of device memory, %.1f GiB are free", (long long)n64,
                   (double)need / 1073741824.0, (double)fre / 1073741824.0);
  if (!A->colptr && (rc = dz_build_transpose(ctx, const_cast<dazim_csr *>(A)))) return rc;
  MtBig big;
  DZ_HIP(dz_malloc_retry(ctx, &big.p[0], bA));
  DZ_HIP(dz_malloc_retry(ctx, &big.p[1], bA));
  if (want_dof) DZ_HIP(dz_malloc_retry(ctx, &big.p[2], bC));
  double *Dd = (double *)big.p[0], *Wd = (double *)big.p[1], *Cd = (double *)big.p[2];
  const int64_t gdata = (m_data + MT_RG - 1) / MT_RG, greg = (mreg + MT_RG - 1) / MT_RG;
  double *g, *y, *part, *rowdot, *sc;
  int64_t *regstart;
  int *flags;
  if ((rc = dz_scratch(ctx, "motrade.g", (size_t)n, &g)) || (rc = dz_scratch(ctx, "motrade.y", (size_t)n, &y)) ||
      (rc = dz_scratch(ctx, "motrade.part", (size_t)std::max<int64_t>(std::max(gdata, greg), 1) * 3, &part)) ||
      (rc = dz_scratch(ctx, "motrade.rowdot", (size_t)n, &rowdot)) || (rc = dz_scratch(ctx, "motrade.sc", (size_t)MT_NSC, &sc)) ||
      (rc = dz_scratch(ctx, "motrade.reg", (size_t)n, &regstart)) || (rc = dz_scratch(ctx, "motrade.flags", (size_t)(2 * K + 2), &flags)))
    return rc;
  DzBuf<float> bb, xo;
  DzBuf<double> o_chi, o_reg, o_xn, o_lda, o_ldp, o_dof, o_gcv, o_lev;
  const size_t kk = (size_t)K;
  if ((rc = bb.init(ctx, b_u, (size_t)m_data, true, false)) || (rc = xo.init(ctx, x_u, x_u ? kk * n : 0, false, true)) ||
      (rc = o_chi.init(ctx, chi2_u, kk, false, true)) || (rc = o_reg.init(ctx, reg2_u, kk * nblk, false, true)) ||
      (rc = o_xn.init(ctx, xnorm2_u, kk, false, true)) || (rc = o_lda.init(ctx, logdet_a_u, kk, false, true)) ||
      (rc = o_ldp.init(ctx, logdet_p_u, logdet_p_u ? kk : 0, false, true)) || (rc = o_dof.init(ctx, dof_u, dof_u ? kk * nblk : 0, false, true)) ||
      (rc = o_gcv.init(ctx, gcv_u, gcv_u ? kk : 0, false, true)) || (rc = o_lev.init(ctx, logev_u, logev_u ? kk : 0, false, true)))
    return rc;
  std::vector<int> hflag((size_t)(2 * K + 2), 0);
  int *bad = flags + 2 * K;
  DZ_HIP(hipMemsetAsync(flags, 0, (size_t)(2 * K + 2) * sizeof(int), ctx->stream));
  if ((rc = dz_mo_check_rows(ctx, A, n, bad))) return rc;
  if (mreg > 0)
    hipLaunchKernelGGL(k_mt_span, dim3((unsigned)((mreg + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, m_data, mreg, maxvp, A->rowptr, A->col, bad + 1);
  DZ_HIP(hipGetLastError());
  DZ_HIP(hipMemcpyAsync(hflag.data() + 2 * K, bad, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (hflag[2 * K]) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: a row's columns do not ascend strictly inside 0..n-1");
  if (hflag[2 * K + 1]) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_model_tradeoff: a regularisation row spans two blocks");
  const bool mfma = dz_opt(ctx, "map_post.mfma", 1) != 0;
  const char *lapname = "model_trade.lap";
  double sec[4] = {0, 0, 0, 0};   // gram, factor, solve, inverse
  auto lap = [&](int which, DzTimer &t) {
    t.stop();
    sec[which] += ctx->ksec[lapname];
  };
  const unsigned nvb = (unsigned)((n + MP_TB - 1) / MP_TB);
  {
    DzTimer t(ctx, lapname);
    if ((rc = dz_mo_regstart(ctx, A, n, m_data, regstart))) return rc;
    hipLaunchKernelGGL(k_mt_gram_data, dim3((unsigned)n), dim3(64), 0, ctx->stream, n, A->colptr, regstart, A->row, A->tval, A->rowptr, A->col, A->val, Dd);
    if ((rc = dz_mt_mirror(ctx, n, Dd))) return rc;
    hipLaunchKernelGGL(k_mt_rhs, dim3((unsigned)n), dim3(64), 0, ctx->stream, A->colptr, regstart, A->row, A->tval, bb.dev, g);
    DZ_HIP(hipMemsetAsync(Wd, 0, bA, ctx->stream));   // (the upper triangle of the work matrix is never written or read)
    DZ_HIP(hipGetLastError());
    lap(0, t);
  }
  const MtOut out = {o_chi.dev, o_reg.dev, o_xn.dev, o_lda.dev, o_ldp.dev, o_dof.dev, o_gcv.dev, o_lev.dev};
  for (int k = 0; k < K; k++) {
    MtScale s;
    for (int b = 0; b < 3; b++) s.s2[b] = b < nblk ? (double)scale[k * nblk + b] * (double)scale[k * nblk + b] : 0.0;
    const double d2 = (double)damp[k] * (double)damp[k];
    int *fl = flags + 2 * k;
    {
      DzTimer t(ctx, lapname);
      hipLaunchKernelGGL(k_mt_combine, dim3((unsigned)n), dim3(64), 0, ctx->stream, n, maxvp, A->colptr, regstart, A->row, A->tval, A->rowptr, A->col,
                         A->val, Dd, s, d2, Wd);
      DZ_HIP(hipGetLastError());
      lap(1, t);
    }
    if ((rc = dz_mp_factor(ctx, n, Wd, fl, mfma, lapname, sec + 1))) return rc;
    {
      DzTimer t(ctx, lapname);
      DZ_HIP(hipMemsetAsync(sc, 0, MT_NSC * sizeof(double), ctx->stream));
      DZ_HIP(hipMemcpyAsync(y, g, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      if ((rc = dz_mt_solve(ctx, n, Wd, y)) || (rc = dz_mt_logdet_norm(ctx, n, Wd, y, sc + MT_LDA, sc + MT_XN))) return rc;
      if (gdata > 0) {
        hipLaunchKernelGGL(k_mt_rows<false>, dim3((unsigned)((gdata + MP_TB / 64 - 1) / (MP_TB / 64))), dim3(MP_TB), 0, ctx->stream, (int64_t)0, m_data,
                           maxvp, A->rowptr, A->col, A->val, y, bb.dev, part);
        if ((rc = dz_mt_sum(ctx, 1, gdata, 3, 1, part, sc + MT_CHI2))) return rc;
      }
      if (greg > 0) {
        hipLaunchKernelGGL(k_mt_rows<true>, dim3((unsigned)((greg + MP_TB / 64 - 1) / (MP_TB / 64))), dim3(MP_TB), 0, ctx->stream, m_data, mreg, maxvp,
                           A->rowptr, A->col, A->val, y, (const float *)nullptr, part);
        if ((rc = dz_mt_sum(ctx, nblk, greg, 3, 1, part, sc + MT_REG2))) return rc;
      }
      if (xo.dev) hipLaunchKernelGGL(k_mt_xout, dim3(nvb), dim3(MP_TB), 0, ctx->stream, n, y, fl, xo.dev + (size_t)k * n);
      DZ_HIP(hipGetLastError());
      lap(2, t);
    }
    if (want_dof) {
      double s3[3] = {0, 0, 0};
      if ((rc = dz_mp_inverse_c(ctx, n, Wd, Cd, mfma, lapname, s3))) return rc;
      DzTimer t(ctx, lapname);
      if ((rc = dz_mt_rowdot(ctx, n, Cd, Dd, rowdot)) || (rc = dz_mt_sum(ctx, nblk, maxvp, 1, maxvp, rowdot, sc + MT_DOF))) return rc;
      lap(3, t);
      sec[3] += s3[1] + s3[2];
    }
    if (want_evidence) {
      {
        DzTimer t(ctx, lapname);
        hipLaunchKernelGGL(k_mt_combine, dim3((unsigned)n), dim3(64), 0, ctx->stream, n, maxvp, A->colptr, regstart, A->row, A->tval, A->rowptr, A->col,
                           A->val, (const double *)nullptr, s, d2, Wd);
        DZ_HIP(hipGetLastError());
        lap(1, t);
      }
      if ((rc = dz_mp_factor(ctx, n, Wd, fl + 1, mfma, lapname, sec + 1))) return rc;
      DzTimer t(ctx, lapname);
      if ((rc = dz_mt_logdet_norm(ctx, n, Wd, nullptr, sc + MT_LDP, nullptr))) return rc;
      lap(1, t);
    }
    hipLaunchKernelGGL(k_mt_final, dim3(1), dim3(1), 0, ctx->stream, k, nblk, m_data, s, d2, want_dof, want_evidence, fl, sc, out);
    DZ_HIP(hipGetLastError());
  }
  DZ_HIP(hipMemcpyAsync(hflag.data(), flags, (size_t)(2 * K) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = xo.finish()) || (rc = o_chi.finish()) || (rc = o_reg.finish()) || (rc = o_xn.finish()) || (rc = o_lda.finish()) || (rc = o_ldp.finish()) ||
      (rc = o_dof.finish()) || (rc = o_gcv.finish()) || (rc = o_lev.finish()))
    return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_failed)
    for (int k = 0; k < K; k++) n_failed[k] = hflag[2 * k] != 0;
  ctx->ksec.erase(lapname);
  static const char *names[4] = {"model_trade.gram", "model_trade.factor", "model_trade.solve", "model_trade.inverse"};
  double total = 0.0;
  for (int i = 0; i < 4; i++) {
    ctx->ksec[names[i]] = sec[i];
    total += sec[i];
  }
  ctx->ksec["model_tradeoff"] = total;
  ctx->ksec["model_trade.points"] = (double)K;
  ctx->ksec["model_trade.n"] = (double)n;
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
