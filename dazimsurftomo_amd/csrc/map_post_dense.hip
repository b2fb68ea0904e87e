// map_post_dense.hip -- the dense fp64 part that dazim_map_posterior (per period) and dazim_model_posterior (once) share, dz_mp_dense
// of map_post_internal.h, and its two halves dz_mp_factor and dz_mp_inverse_c, which dazim_model_tradeoff calls per sweep point: on one
// block of ng unknowns
//   factor   blocked right-looking Cholesky in place, panel width MP_NB: diagonal block, panel solve, trailing update
//   inverse  M = R^-1 in place, block column by block column from the last: diagonal block, M22 * R21 into the second matrix, -(.) * M11
//   c        C = M^T M into the second matrix, both triangles
// Every sum in a fixed order, no floating-point atomics; the dependencies between the steps are launch order on the context's stream.
// The trailing update and C have two tile forms: plain VALU arithmetic and v_mfma_f64_16x16x4_f64.
#include <algorithm>

#include "map_post_internal.h"

namespace {

// ---- factor ----------------------------------------------------------------------------------------------------------------------
// diagonal block [k0, k0 + nb): right-looking Cholesky in LDS, the order of dz_column_solve; flag = 1 at a pivot not finite and > 0
__global__ __launch_bounds__(MP_TB) void k_mp_potrf(int ng, int k0, int nb, double *A, int *flag) {
  __shared__ double S[MP_NB][MP_NB + 1];
  const int t = threadIdx.x;
  for (int q = t; q < nb * nb; q += MP_TB) {
    const int i = q / nb, j = q - i * nb;
    if (j <= i) S[i][j] = A[(size_t)(k0 + i) * ng + k0 + j];
  }
  __syncthreads();
  bool ok = true;
  for (int c = 0; c < nb; c++) {
    const double pv = S[c][c];
    ok = ok && isfinite(pv) && pv > 0.0;
    const double d = sqrt(pv);
    __syncthreads();
    if (t > c && t < nb) S[t][c] /= d;
    if (t == c) S[c][c] = d;
    __syncthreads();
    const int mm = nb - c - 1;
    for (int q = t; q < mm * mm; q += MP_TB) {
      const int i = c + 1 + q / mm, j = c + 1 + q % mm;
      if (j <= i) S[i][j] -= S[i][c] * S[j][c];
    }
    __syncthreads();
  }
  for (int q = t; q < nb * nb; q += MP_TB) {
    const int i = q / nb, j = q - i * nb;
    if (j <= i) A[(size_t)(k0 + i) * ng + k0 + j] = S[i][j];
  }
  if (t == 0 && !ok) *flag = 1;
}

// panel below the diagonal block: row i, A[i][k0 + c] = (A[i][k0 + c] - sum_{j < c} A[i][k0 + j] R[c][j]) / R[c][c], ascending j
__global__ __launch_bounds__(MP_TB) void k_mp_trsm(int ng, int k0, int nb, double *A) {
  __shared__ double S[MP_NB][MP_NB + 1];
  const int t = threadIdx.x;
  for (int q = t; q < nb * nb; q += MP_TB) {
    const int i = q / nb, j = q - i * nb;
    if (j <= i) S[i][j] = A[(size_t)(k0 + i) * ng + k0 + j];
  }
  __syncthreads();
  const int i = k0 + nb + blockIdx.x * MP_TB + t;
  if (i >= ng) return;
  double *Ai = A + (size_t)i * ng + k0;
  double x[MP_NB];
#pragma unroll
  for (int c = 0; c < MP_NB; c++) {
    if (c < nb) {
      double s = Ai[c];
#pragma unroll
      for (int j = 0; j < c; j++) s -= x[j] * S[c][j];
      x[c] = s / S[c][c];
      Ai[c] = x[c];
    }
  }
}

// trailing update: A[i][j] -= sum_{p in the panel} A[i][k0 + p] A[j][k0 + p], ascending p, for k0 + nb <= j <= i
template <class F>
__global__ __launch_bounds__(MP_TB) void k_mp_syrk(int ng, int k0, int nb, double *A) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ double As[MP_NB][MP_LD], Bs[MP_NB][MP_LD];
  const int t = threadIdx.x, s0 = k0 + nb, i0 = s0 + blockIdx.y * MP_TS, j0 = s0 + blockIdx.x * MP_TS;
  for (int q = t; q < MP_TS * MP_NB; q += MP_TB) {
    const int ii = q / MP_NB, p = q % MP_NB;
    As[p][ii] = (p < nb && i0 + ii < ng) ? A[(size_t)(i0 + ii) * ng + k0 + p] : 0.0;
    Bs[p][ii] = (p < nb && j0 + ii < ng) ? A[(size_t)(j0 + ii) * ng + k0 + p] : 0.0;
  }
  __syncthreads();
  F f(t);
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int i = i0 + f.row(u, v), j = j0 + f.colof(u, v);
      f.acc[u][v] = (i < ng && j <= i) ? A[(size_t)i * ng + j] : 0.0;
    }
  f.template slab<true>(As, Bs, nb);
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int i = i0 + f.row(u, v), j = j0 + f.colof(u, v);
      if (i < ng && j <= i) A[(size_t)i * ng + j] = f.acc[u][v];
    }
}

// ---- inverse ---------------------------------------------------------------------------------------------------------------------
// diagonal block [jb, jb + nb) in place: column k of its inverse by forward substitution on e_k (thread k), the order of
// dz_column_inverse_factor
__global__ __launch_bounds__(64) void k_mp_trtri(int ng, int jb, int nb, double *A) {
  __shared__ double S[MP_NB][MP_NB + 1], Y[MP_NB][MP_NB + 1];
  const int t = threadIdx.x;
  for (int q = t; q < nb * nb; q += 64) {
    const int i = q / nb, j = q - i * nb;
    if (j <= i) S[i][j] = A[(size_t)(jb + i) * ng + jb + j];
  }
  __syncthreads();
  if (t < nb) {
    const int k = t;
    Y[k][k] = 1.0 / S[k][k];
    for (int i = k + 1; i < nb; i++) {
      double s = S[i][k] * Y[k][k];
      for (int j = k + 1; j < i; j++) s += S[i][j] * Y[j][k];
      Y[i][k] = -s / S[i][i];
    }
  }
  __syncthreads();
  for (int q = t; q < nb * nb; q += 64) {
    const int i = q / nb, j = q - i * nb;
    if (j <= i) A[(size_t)(jb + i) * ng + jb + j] = Y[i][j];
  }
}

// W[i][c] = sum_{l = s0 .. i} M[i][l] R[l][jb + c], ascending l, for s0 = jb + nb <= i < ng: the inverted trailing block times the
// panel below the diagonal block.  W [ng][MP_NB].  MP_TS rows per workgroup; thread (ty, tx) holds rows ty + 16u, columns tx + 16v.
__global__ __launch_bounds__(MP_TB) void k_mp_inv_mm(int ng, int jb, int nb, const double *A, double *W) {
  __shared__ double As[MP_NB][MP_LD], Bs[MP_NB][MP_NB + 1];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15, s0 = jb + nb, i0 = s0 + blockIdx.x * MP_TS;
  double acc[4][2] = {};
  const int lend = min(i0 + MP_TS, ng);
  // the next slab travels from memory into registers while this one is multiplied: the k loop of a workgroup is a chain of up to
  // n_g / MP_NB slabs, and few workgroups run beside it
  double ra[MP_TS * MP_NB / MP_TB], rb[MP_NB * MP_NB / MP_TB];
  auto fetch = [&](int l0) {
#pragma unroll
    for (int u = 0; u < MP_TS * MP_NB / MP_TB; u++) {
      const int q = t + u * MP_TB, ii = q / MP_NB, k = q % MP_NB, i = i0 + ii, l = l0 + k;
      ra[u] = (i < ng && l <= i) ? A[(size_t)i * ng + l] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < MP_NB * MP_NB / MP_TB; u++) {
      const int q = t + u * MP_TB, k = q / MP_NB, c = q % MP_NB, l = l0 + k;
      rb[u] = (l < ng && c < nb) ? A[(size_t)l * ng + jb + c] : 0.0;
    }
  };
  fetch(s0);
  for (int l0 = s0; l0 < lend; l0 += MP_NB) {
#pragma unroll
    for (int u = 0; u < MP_TS * MP_NB / MP_TB; u++) {
      const int q = t + u * MP_TB;
      As[q % MP_NB][q / MP_NB] = ra[u];
    }
#pragma unroll
    for (int u = 0; u < MP_NB * MP_NB / MP_TB; u++) {
      const int q = t + u * MP_TB;
      Bs[q / MP_NB][q % MP_NB] = rb[u];
    }
    __syncthreads();
    if (l0 + MP_NB < lend) fetch(l0 + MP_NB);
    for (int k = 0; k < MP_NB; k++) {
      const double b0 = Bs[k][tx], b1 = Bs[k][tx + 16];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const double a = As[k][ty + 16 * u];
        acc[u][0] += a * b0;
        acc[u][1] += a * b1;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 2; v++) {
      const int i = i0 + ty + 16 * u, c = tx + 16 * v;
      if (i < ng && c < nb) W[(size_t)i * MP_NB + c] = acc[u][v];
    }
}

// A[i][jb + c] = -sum_{e = c .. nb-1} W[i][e] M11[e][c], ascending e (M11 the inverted diagonal block), one thread per row i
__global__ __launch_bounds__(MP_TB) void k_mp_inv_scale(int ng, int jb, int nb, double *A, const double *W) {
  __shared__ double S[MP_NB][MP_NB + 1];
  const int t = threadIdx.x;
  for (int q = t; q < nb * nb; q += MP_TB) {
    const int i = q / nb, j = q - i * nb;
    if (j <= i) S[i][j] = A[(size_t)(jb + i) * ng + jb + j];
  }
  __syncthreads();
  const int i = jb + nb + blockIdx.x * MP_TB + t;
  if (i >= ng) return;
  const double *Wi = W + (size_t)i * MP_NB;
  for (int c = 0; c < nb; c++) {
    double s = 0.0;
    for (int e = c; e < nb; e++) s += Wi[e] * S[e][c];
    A[(size_t)i * ng + jb + c] = -s;
  }
}

// ---- C = M^T M: C_ac = sum_{i >= max(a, c)} M_ia M_ic, ascending i; tile (a, c) with c's tile <= a's, both triangles written --------
template <class F>
__global__ __launch_bounds__(MP_TB) void k_mp_ctc(int ng, const double *M, double *Cm) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ double As[MP_NB][MP_LD], Bs[MP_NB][MP_LD];
  const int t = threadIdx.x, a0 = blockIdx.y * MP_TS, c0 = blockIdx.x * MP_TS;
  F f(t);
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) f.acc[u][v] = 0.0;
  for (int i0 = a0; i0 < ng; i0 += MP_NB) {
    for (int q = t; q < MP_TS * MP_NB; q += MP_TB) {
      const int k = q / MP_TS, aa = q % MP_TS, i = i0 + k;
      As[k][aa] = (i < ng && a0 + aa <= i) ? M[(size_t)i * ng + a0 + aa] : 0.0;
      Bs[k][aa] = (i < ng && c0 + aa <= i) ? M[(size_t)i * ng + c0 + aa] : 0.0;
    }
    __syncthreads();
    f.template slab<false>(As, Bs, MP_NB);
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int a = a0 + f.row(u, v), c = c0 + f.colof(u, v);
      if (a < ng && c <= a) {
        Cm[(size_t)a * ng + c] = f.acc[u][v];
        Cm[(size_t)c * ng + a] = f.acc[u][v];
      }
    }
}

}  // namespace

int dz_mp_factor(dazim_ctx *ctx, int ng, double *Ad, int *flag, bool mfma, const char *lapname, double *sec) {
  DzTimer t(ctx, lapname);
  for (int k0 = 0; k0 < ng; k0 += MP_NB) {
    const int nb = std::min(MP_NB, ng - k0), rest = ng - k0 - nb;
    hipLaunchKernelGGL(k_mp_potrf, dim3(1), dim3(MP_TB), 0, ctx->stream, ng, k0, nb, Ad, flag);
    if (rest > 0) {
      const unsigned nt = (unsigned)((rest + MP_TS - 1) / MP_TS);
      hipLaunchKernelGGL(k_mp_trsm, dim3((unsigned)((rest + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, ng, k0, nb, Ad);
      if (mfma) hipLaunchKernelGGL(k_mp_syrk<MpMfma>, dim3(nt, nt), dim3(MP_TB), 0, ctx->stream, ng, k0, nb, Ad);
      else hipLaunchKernelGGL(k_mp_syrk<MpPlain>, dim3(nt, nt), dim3(MP_TB), 0, ctx->stream, ng, k0, nb, Ad);
    }
  }
  DZ_HIP(hipGetLastError());
  t.lap(sec[0]);
  return 0;
}

int dz_mp_inverse_c(dazim_ctx *ctx, int ng, double *Ad, double *Cd, bool mfma, const char *lapname, double *sec) {
  {
    DzTimer t(ctx, lapname);
    for (int jb = ((ng - 1) / MP_NB) * MP_NB; jb >= 0; jb -= MP_NB) {
      const int nb = std::min(MP_NB, ng - jb), rest = ng - jb - nb;
      hipLaunchKernelGGL(k_mp_trtri, dim3(1), dim3(64), 0, ctx->stream, ng, jb, nb, Ad);
      if (rest > 0) {
        hipLaunchKernelGGL(k_mp_inv_mm, dim3((unsigned)((rest + MP_TS - 1) / MP_TS)), dim3(MP_TB), 0, ctx->stream, ng, jb, nb, Ad, Cd);
        hipLaunchKernelGGL(k_mp_inv_scale, dim3((unsigned)((rest + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, ng, jb, nb, Ad, Cd);
      }
    }
    DZ_HIP(hipGetLastError());
    t.lap(sec[1]);
  }
  {
    DzTimer t(ctx, lapname);
    const unsigned nt = (unsigned)((ng + MP_TS - 1) / MP_TS);
    if (mfma) hipLaunchKernelGGL(k_mp_ctc<MpMfma>, dim3(nt, nt), dim3(MP_TB), 0, ctx->stream, ng, Ad, Cd);
    else hipLaunchKernelGGL(k_mp_ctc<MpPlain>, dim3(nt, nt), dim3(MP_TB), 0, ctx->stream, ng, Ad, Cd);
    DZ_HIP(hipGetLastError());
    t.lap(sec[2]);
  }
  return 0;
}

int dz_mp_dense(dazim_ctx *ctx, int ng, double *Ad, double *Cd, int *flag, bool mfma, const char *lapname, double *sec) {
  const int rc = dz_mp_factor(ctx, ng, Ad, flag, mfma, lapname, sec);
  return rc ? rc : dz_mp_inverse_c(ctx, ng, Ad, Cd, mfma, lapname, sec);
}
