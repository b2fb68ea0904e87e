// map_post.hip -- dazim_map_posterior: posterior std and resolution of the per-period maps from the matrix LSMR
// is given, [W G; L], and the damping.  The normal matrix is block diagonal by period; per period (group) of n_g unknowns:
//   gram     A_g = sum_rows r^T r + damp^2 I, one wavefront per row of A_g over the period's sparse rows in ascending order
//   factor   blocked right-looking Cholesky in place, panel width MP_NB: diagonal block, panel solve, trailing update
//   inverse  M = R^-1 in place, block column by block column from the last: diagonal block, M22 * R21 into the second matrix, -(.) * M11
//   c        C = M^T M into the second matrix, both triangles
//   rows     one workgroup per row of Rm = I - C P with the regularisation rows as they are, and every per-unknown output
// fp64, every sum in a fixed order, no floating-point atomics; the dependencies between the steps are launch order on the context's
// stream.  The trailing update and C have two tile forms: plain VALU arithmetic and v_mfma_f64_16x16x4_f64 (option map_post.mfma).
#include <algorithm>
#include <cmath>

#include "sparse_internal.h"

namespace {

constexpr int MP_NB = 32;   // panel width of the factorisation and of the inverse (stat map_post.nb)
constexpr int MP_TS = 64;   // the tile kernels' output tile, MP_TS x MP_TS per workgroup of MP_TB threads
constexpr int MP_TB = 256;
constexpr int MP_LD = MP_TS + 1;
constexpr int MP_EMAX = 8;  // entries of a regularisation row the row pass keeps in LDS (a longer row is read from memory again)

typedef double mp_v4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int mp_local(int c, int kn, int ncell) { return (c / kn) * ncell + c % ncell; }

// period of every row (-1: a row without entries) and the range of cells it touches, span[2r] .. span[2r+1]; bad |= 1 for a row whose
// columns lie in two periods, |= 2 for a row whose columns do not ascend strictly
__global__ __launch_bounds__(MP_TB) void k_mp_row_period(int64_t m, const int64_t *rowptr, const int *col, int kn, int ncell, int *per,
                                                         int *span, int *bad) {
  const int64_t r = (int64_t)blockIdx.x * MP_TB + threadIdx.x;
  if (r >= m) return;
  int p = -1, prev = -1, b = 0, lo = ncell, hi = -1;
  for (int64_t q = rowptr[r]; q < rowptr[r + 1]; q++) {
    const int c = col[q], pp = (c % kn) / ncell, cell = c % ncell;
    if (p < 0) p = pp;
    else if (pp != p) b |= 1;
    if (c <= prev) b |= 2;
    prev = c;
    lo = min(lo, cell);
    hi = max(hi, cell);
  }
  per[r] = p;
  span[2 * r] = lo;
  span[2 * r + 1] = hi;
  if (b) atomicOr(bad, b);
}

// block p: the rows of period p in ascending order.  list == NULL: cnt[2p] = their number, cnt[2p+1] = how many are data rows;
// otherwise the rows go to list + sum_{q<p} cnt[2q]
__global__ __launch_bounds__(MP_TB) void k_mp_row_lists(int64_t m, int64_t m_data, const int *per, int *cnt, int *list) {
  __shared__ int ws[MP_TB / 64], wd[MP_TB / 64];
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  int base = 0, based = 0, off = 0;
  if (list)
    for (int q = 0; q < p; q++) off += cnt[2 * q];
  for (int64_t r0 = 0; r0 < m; r0 += MP_TB) {
    const int64_t r = r0 + t;
    const bool f = r < m && per[r] == p;
    const unsigned long long bf = __ballot(f), bd = __ballot(f && r < m_data);
    if (lane == 0) {
      ws[w] = __popcll(bf);
      wd[w] = __popcll(bd);
    }
    __syncthreads();
    int wb = 0, tot = 0, totd = 0;
    for (int i = 0; i < MP_TB / 64; i++) {
      if (i < w) wb += ws[i];
      tot += ws[i];
      totd += wd[i];
    }
    if (f && list) list[off + base + wb + __popcll(bf & ((1ull << lane) - 1ull))] = (int)r;
    base += tot;
    based += totd;
    __syncthreads();
  }
  if (!list && t == 0) {
    cnt[2 * p] = base;
    cnt[2 * p + 1] = based;
  }
}

// row a of A_g (all n_g entries; the lower triangle is what the factorisation reads): sum over the period's rows r, ascending, of
// r_a r_c, then damp^2 on the diagonal.  One wavefront per row a; a row of the matrix holds column a at most once.  Of 64 rows at a
// time only those whose range of cells holds a's cell are read (a map row has about 130 of 2 704 cells, close together).
__global__ __launch_bounds__(64) void k_mp_gram(int ng, int ncell, int kn, int p, int nrow, const int *list, const int *span,
                                                const int64_t *rowptr, const int *col, const float *val, double d2, double *A) {
  const int a = blockIdx.x, t = threadIdx.x, cell_a = a % ncell;
  const int ga = (a / ncell) * kn + p * ncell + a % ncell;
  double *Aa = A + (size_t)a * ng;
  for (int c = t; c < ng; c += 64) Aa[c] = 0.0;
  __syncthreads();
  for (int i0 = 0; i0 < nrow; i0 += 64) {
    long long mb = 0, me = 0;
    bool near = false;
    if (i0 + t < nrow) {
      const int r = list[i0 + t];
      mb = rowptr[r];
      me = rowptr[r + 1];
      near = span[2 * (size_t)r] <= cell_a && cell_a <= span[2 * (size_t)r + 1];
    }
    for (unsigned long long cand = __ballot(near); cand; cand &= cand - 1ull) {   // ascending rows
      const int k = __ffsll((long long)cand) - 1;
      const long long b = __shfl(mb, k), e = __shfl(me, k);
      float va = 0.0f;
      bool hit = false;
      for (long long q = b + t; q < e; q += 64)
        if (col[q] == ga) {
          va = val[q];
          hit = true;
        }
      const unsigned long long h = __ballot(hit);
      if (!h) continue;
      const double v = (double)__shfl(va, __ffsll((long long)h) - 1);
      for (long long q = b + t; q < e; q += 64) {
        const int lc = mp_local(col[q], kn, ncell);
        if (lc <= a) Aa[lc] += v * (double)val[q];
      }
      __syncthreads();   // (the next row may hold the same columns in other lanes)
    }
  }
  if (t == 0) Aa[a] += d2;
}

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

// the two tile forms of acc (+/-)= sum_k As[k][i] Bs[k][j] over a k-major pair of LDS slabs of MP_NB rows.
// plain: thread (ty, tx) holds rows ty + 16u, columns tx + 16v.  mfma: wavefront w holds rows 16w .. 16w+15 as four 16 x 16 blocks,
// lane l of block cb element reg at row (l >> 4) + 4 reg, column 16 cb + (l & 15); the A operand is negated for a subtraction.
struct MpPlain {
  double acc[4][4];
  int ty, tx;
  __device__ __forceinline__ MpPlain(int t) : ty(t >> 4), tx(t & 15) {}
  __device__ __forceinline__ int row(int u, int) const { return ty + 16 * u; }
  __device__ __forceinline__ int colof(int, int v) const { return tx + 16 * v; }
  template <bool SUB>
  __device__ __forceinline__ void slab(const double (*As)[MP_LD], const double (*Bs)[MP_LD], int nk) {
    for (int k = 0; k < nk; k++) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; u++) a[u] = As[k][ty + 16 * u];
#pragma unroll
      for (int v = 0; v < 4; v++) b[v] = Bs[k][tx + 16 * v];
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
          if (SUB) acc[u][v] -= a[u] * b[v];
          else acc[u][v] += a[u] * b[v];
        }
    }
  }
};
struct MpMfma {
  double acc[4][4];   // [reg][cb]
  int w, l;
  __device__ __forceinline__ MpMfma(int t) : w(t >> 6), l(t & 63) {}
  __device__ __forceinline__ int row(int u, int) const { return 16 * w + (l >> 4) + 4 * u; }
  __device__ __forceinline__ int colof(int, int v) const { return 16 * v + (l & 15); }
  template <bool SUB>
  __device__ __forceinline__ void slab(const double (*As)[MP_LD], const double (*Bs)[MP_LD], int) {   // (rows nk .. MP_NB-1 hold 0)
    mp_v4 d[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
      for (int r = 0; r < 4; r++) d[cb][r] = acc[r][cb];
#pragma unroll
    for (int k0 = 0; k0 < MP_NB; k0 += 4) {
      const double a0 = As[k0 + (l >> 4)][16 * w + (l & 15)], a = SUB ? -a0 : a0;
#pragma unroll
      for (int cb = 0; cb < 4; cb++) d[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[k0 + (l >> 4)][16 * cb + (l & 15)], d[cb], 0, 0, 0);
    }
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r][cb] = d[cb][r];
  }
};

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

// ---- row pass ----------------------------------------------------------------------------------------------------------------------
// the sums of a workgroup's threads in a fixed order: butterfly inside a wavefront, the wavefronts' values in ascending order
__device__ __forceinline__ double mp_block_sum(double v, double *red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < MP_TB / 64; i++) s += red[i];
  return s;
}

struct MpOut {
  float *std_post, *std_noise, *rdiag, *rsum, *width, *leak, *rows;
};

// workgroup a: Rm_a. = e_a - sum_l (C_a. l) l - damp^2 C_a. over the period's regularisation rows l in ascending order, and what is
// summed along that row.  Dynamic LDS: rm [ng] | tb [MP_TB] | eval [MP_TB][MP_EMAX] | ebeg [MP_TB] | ecol [MP_TB][MP_EMAX] | elen [MP_TB]
__global__ __launch_bounds__(MP_TB) void k_mp_rows(int ng, int ncell, int nvx, int kn, int p, int nreg, const int *reglist,
                                                   const int64_t *rowptr, const int *col, const float *val, double d2, const double *Cm,
                                                   const int *flag, MpOut out, int nsel, const int *sel, double *rd64) {
  extern __shared__ double sm[];
  __shared__ double red[MP_TB / 64];
  double *rm = sm, *tb = rm + ng, *eval = tb + MP_TB;
  long long *ebeg = (long long *)(eval + MP_TB * MP_EMAX);
  int *ecol = (int *)(ebeg + MP_TB), *elen = ecol + MP_TB * MP_EMAX;
  const int a = blockIdx.x, t = threadIdx.x;
  const int blk = a / ncell, cell = a % ncell;
  const size_t o = (size_t)blk * kn + (size_t)p * ncell + cell;
  if (*flag) {
    const float v = nanf("");
    if (t == 0) {
      out.std_post[o] = out.std_noise[o] = out.rdiag[o] = out.rsum[o] = v;
      if (out.width) out.width[o] = v;
      if (out.leak) out.leak[o] = v;
      rd64[a] = (double)v;
    }
    if (out.rows)
      for (int s = 0; s < nsel; s++)
        if (sel[s] == a)
          for (int c = t; c < ng; c += MP_TB) out.rows[((size_t)p * nsel + s) * ng + c] = v;
    return;
  }
  const double *Ca = Cm + (size_t)a * ng;
  for (int c = t; c < ng; c += MP_TB) rm[c] = c == a ? 1.0 : 0.0;
  __syncthreads();
  for (int k0 = 0; k0 < nreg; k0 += MP_TB) {
    if (k0 + t < nreg) {
      const int r = reglist[k0 + t];
      const long long b = rowptr[r], e = rowptr[r + 1];
      double s = 0.0;
      for (long long q = b; q < e; q++) {
        const int lc = mp_local(col[q], kn, ncell);
        const double v = (double)val[q];
        s += Ca[lc] * v;
        if (q - b < MP_EMAX) {
          ecol[t * MP_EMAX + (int)(q - b)] = lc;
          eval[t * MP_EMAX + (int)(q - b)] = v;
        }
      }
      tb[t] = s;
      ebeg[t] = b;
      elen[t] = (int)(e - b);
    }
    __syncthreads();
    if (t < 64) {                                   // one wavefront: its LDS operations take effect in program order
      const int nk = min(MP_TB, nreg - k0);
      for (int k = 0; k < nk; k++) {
        const double tt = tb[k];
        const int len = elen[k];
        if (len <= MP_EMAX) {
          if (t < len) rm[ecol[k * MP_EMAX + t]] -= tt * eval[k * MP_EMAX + t];
        } else {
          const long long b = ebeg[k];
          for (int q = t; q < len; q += 64) rm[mp_local(col[b + q], kn, ncell)] -= tt * (double)val[b + q];
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
  }
  for (int c = t; c < ng; c += MP_TB) rm[c] -= d2 * Ca[c];
  __syncthreads();
  const int ia = cell % nvx, ja = cell / nvx;
  double rs = 0.0, nv = 0.0, own = 0.0, oth = 0.0, num = 0.0;
  for (int c = t; c < ng; c += MP_TB) {
    const double r = rm[c];
    rs += r;
    nv += r * Ca[c];
    if (c / ncell == blk) {
      const int cc = c % ncell;
      const double di = (double)(cc % nvx - ia), dj = (double)(cc / nvx - ja);
      own += r * r;
      num += r * r * (di * di + dj * dj);
    } else {
      oth += r * r;
    }
  }
  rs = mp_block_sum(rs, red);
  nv = mp_block_sum(nv, red);
  own = mp_block_sum(own, red);
  oth = mp_block_sum(oth, red);
  num = mp_block_sum(num, red);
  if (t == 0) {
    out.std_post[o] = (float)sqrt(Ca[a]);
    out.std_noise[o] = (float)sqrt(fmax(nv, 0.0));
    out.rdiag[o] = (float)rm[a];
    out.rsum[o] = (float)rs;
    if (out.width) out.width[o] = own > 0.0 ? (float)sqrt(num / own) : 0.0f;
    if (out.leak) out.leak[o] = own + oth > 0.0 ? (float)(oth / (own + oth)) : 0.0f;
    rd64[a] = rm[a];
  }
  if (out.rows)
    for (int s = 0; s < nsel; s++)
      if (sel[s] == a)
        for (int c = t; c < ng; c += MP_TB) out.rows[((size_t)p * nsel + s) * ng + c] = (float)rm[c];
}

// trace[blk][p] = sum of Rm_aa over the block's cells (workgroup blk)
__global__ __launch_bounds__(MP_TB) void k_mp_trace(int ncell, int kmax, int p, const double *rd64, float *trace) {
  __shared__ double red[MP_TB / 64];
  const int blk = blockIdx.x;
  double s = 0.0;
  for (int c = threadIdx.x; c < ncell; c += MP_TB) s += rd64[(size_t)blk * ncell + c];
  s = mp_block_sum(s, red);
  if (threadIdx.x == 0) trace[blk * kmax + p] = (float)s;
}

}  // namespace

extern "C" int dazim_map_posterior(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, int nx, int ny, int kmax, int azim, float damp,
                                   float *std_post_u, float *std_noise_u, float *rdiag_u, float *rsum_u, float *width_u, float *leak_u,
                                   int nsel, const int *sel_u, float *rows_u, float *trace_u, int *n_failed) {
  if (!ctx || !A || nx < 3 || ny < 3 || kmax < 1 || !std_post_u || !std_noise_u || !rdiag_u || !rsum_u)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_map_posterior");
  if (m_data < 0 || m_data > A->m) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: m_data %lld outside 0..%lld", (long long)m_data, (long long)A->m);
  const int nblk = azim ? 3 : 1;
  const int64_t ncell64 = (int64_t)(nx - 2) * (ny - 2), ng64 = nblk * ncell64;
  if (A->n != ng64 * kmax)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: n %lld is not nblk * kmax * ncell = %lld", (long long)A->n, (long long)(ng64 * kmax));
  if (!azim && leak_u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: leak without azim");
  if (!(damp >= 0.0f) || !std::isfinite(damp)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: damp negative or not finite");
  if (nsel < 0 || (nsel > 0 && !sel_u)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: nsel without sel");
  if (rows_u && nsel < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: rows without sel");
  const size_t lds = (size_t)ng64 * 8 + (size_t)MP_TB * (8 + MP_EMAX * 8 + 8 + MP_EMAX * 4 + 4);
  if (lds > 160 * 1024) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: %lld unknowns per period do not fit the row pass's LDS", (long long)ng64);
  DZ_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = dz_join_aux(ctx))) return rc;
  const int ncell = (int)ncell64, ng = (int)ng64, kn = kmax * ncell, nvx = nx - 2;
  const int64_t m = A->m;
  const size_t no = (size_t)ng * kmax;
  // ---- the workspace, all of it before the first launch ----
  double *Ad, *Cd, *rd64;
  int *per, *span, *cnt, *list, *flags;
  if ((rc = dz_scratch(ctx, "mpost.A", (size_t)ng * ng, &Ad)) || (rc = dz_scratch(ctx, "mpost.C", (size_t)ng * (ng > MP_NB ? ng : MP_NB), &Cd)) ||
      (rc = dz_scratch(ctx, "mpost.rd", (size_t)ng, &rd64)) || (rc = dz_scratch(ctx, "mpost.per", (size_t)m, &per)) || (rc = dz_scratch(ctx, "mpost.span", (size_t)2 * m, &span)) ||
      (rc = dz_scratch(ctx, "mpost.list", (size_t)m, &list)) || (rc = dz_scratch(ctx, "mpost.cnt", (size_t)2 * kmax + 1, &cnt)) ||
      (rc = dz_scratch(ctx, "mpost.flags", (size_t)kmax, &flags)))
    return rc;
  DzBuf<float> sp, sn, rd, rs, wd, lk, rw, tr;
  DzBuf<int> sel;
  if ((rc = sel.init(ctx, sel_u, (size_t)nsel, true, false)) || (rc = sp.init(ctx, std_post_u, no, false, true)) ||
      (rc = sn.init(ctx, std_noise_u, no, false, true)) || (rc = rd.init(ctx, rdiag_u, no, false, true)) ||
      (rc = rs.init(ctx, rsum_u, no, false, true)) || (rc = wd.init(ctx, width_u, width_u ? no : 0, false, true)) ||
      (rc = lk.init(ctx, leak_u, leak_u ? no : 0, false, true)) ||
      (rc = rw.init(ctx, rows_u, rows_u ? (size_t)kmax * nsel * ng : 0, false, true)) ||
      (rc = tr.init(ctx, trace_u, trace_u ? (size_t)nblk * kmax : 0, false, true)))
    return rc;
  DZ_HIP(hipFuncSetAttribute((const void *)k_mp_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (a refusal ends the call: no launch)
  if (nsel > 0 && (rc = dz_check_range(ctx, sel.dev, nsel, 0, ng - 1, "dazim_map_posterior: sel"))) return rc;
  // ---- the rows of every period ----
  int *bad = cnt + 2 * kmax, hbad = 0;
  DZ_HIP(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
  DZ_HIP(hipMemsetAsync(flags, 0, (size_t)kmax * sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_mp_row_period, dim3((unsigned)((m + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, m, A->rowptr, A->col, kn, ncell,
                     per, span, bad);
  DZ_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mp_row_lists, dim3((unsigned)kmax), dim3(MP_TB), 0, ctx->stream, m, m_data, per, cnt, (int *)nullptr);
  DZ_HIP(hipGetLastError());
  std::vector<int> hcnt(2 * kmax + 1);
  DZ_HIP(hipMemcpyAsync(hcnt.data(), cnt, hcnt.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  hbad = hcnt[2 * kmax];
  if (hbad & 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: a row's columns lie in two periods");
  if (hbad & 2) return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_map_posterior: a row's columns do not ascend strictly");
  hipLaunchKernelGGL(k_mp_row_lists, dim3((unsigned)kmax), dim3(MP_TB), 0, ctx->stream, m, m_data, per, cnt, list);
  DZ_HIP(hipGetLastError());
  const bool mfma = dz_opt(ctx, "map_post.mfma", 1) != 0;
  const double d2 = (double)damp * (double)damp;
  const MpOut out = {sp.dev, sn.dev, rd.dev, rs.dev, wd.dev, lk.dev, rw.dev};
  double sec[5] = {0, 0, 0, 0, 0};
  auto lap = [&](int which, DzTimer &t) {
    t.stop();
    sec[which] += ctx->ksec["map_post.lap"];
  };
  int off = 0;
  for (int p = 0; p < kmax; p++) {
    const int nrow = hcnt[2 * p], ndat = hcnt[2 * p + 1];
    const int *lp = list + off;
    off += nrow;
    {
      DzTimer t(ctx, "map_post.lap");
      hipLaunchKernelGGL(k_mp_gram, dim3((unsigned)ng), dim3(64), 0, ctx->stream, ng, ncell, kn, p, nrow, lp, span, A->rowptr, A->col, A->val, d2, Ad);
      DZ_HIP(hipGetLastError());
      lap(0, t);
    }
    {
      DzTimer t(ctx, "map_post.lap");
      for (int k0 = 0; k0 < ng; k0 += MP_NB) {
        const int nb = std::min(MP_NB, ng - k0), rest = ng - k0 - nb;
        hipLaunchKernelGGL(k_mp_potrf, dim3(1), dim3(MP_TB), 0, ctx->stream, ng, k0, nb, Ad, flags + p);
        if (rest > 0) {
          const unsigned nt = (unsigned)((rest + MP_TS - 1) / MP_TS);
          hipLaunchKernelGGL(k_mp_trsm, dim3((unsigned)((rest + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, ng, k0, nb, Ad);
          if (mfma) hipLaunchKernelGGL(k_mp_syrk<MpMfma>, dim3(nt, nt), dim3(MP_TB), 0, ctx->stream, ng, k0, nb, Ad);
          else hipLaunchKernelGGL(k_mp_syrk<MpPlain>, dim3(nt, nt), dim3(MP_TB), 0, ctx->stream, ng, k0, nb, Ad);
        }
      }
      DZ_HIP(hipGetLastError());
      lap(1, t);
    }
    {
      DzTimer t(ctx, "map_post.lap");
      for (int jb = ((ng - 1) / MP_NB) * MP_NB; jb >= 0; jb -= MP_NB) {
        const int nb = std::min(MP_NB, ng - jb), rest = ng - jb - nb;
        hipLaunchKernelGGL(k_mp_trtri, dim3(1), dim3(64), 0, ctx->stream, ng, jb, nb, Ad);
        if (rest > 0) {
          hipLaunchKernelGGL(k_mp_inv_mm, dim3((unsigned)((rest + MP_TS - 1) / MP_TS)), dim3(MP_TB), 0, ctx->stream, ng, jb, nb, Ad, Cd);
          hipLaunchKernelGGL(k_mp_inv_scale, dim3((unsigned)((rest + MP_TB - 1) / MP_TB)), dim3(MP_TB), 0, ctx->stream, ng, jb, nb, Ad, Cd);
        }
      }
      DZ_HIP(hipGetLastError());
      lap(2, t);
    }
    {
      DzTimer t(ctx, "map_post.lap");
      const unsigned nt = (unsigned)((ng + MP_TS - 1) / MP_TS);
      if (mfma) hipLaunchKernelGGL(k_mp_ctc<MpMfma>, dim3(nt, nt), dim3(MP_TB), 0, ctx->stream, ng, Ad, Cd);
      else hipLaunchKernelGGL(k_mp_ctc<MpPlain>, dim3(nt, nt), dim3(MP_TB), 0, ctx->stream, ng, Ad, Cd);
      DZ_HIP(hipGetLastError());
      lap(3, t);
    }
    {
      DzTimer t(ctx, "map_post.lap");
      hipLaunchKernelGGL(k_mp_rows, dim3((unsigned)ng), dim3(MP_TB), lds, ctx->stream, ng, ncell, nvx, kn, p, nrow - ndat, lp + ndat, A->rowptr,
                         A->col, A->val, d2, Cd, flags + p, out, nsel, sel.dev, rd64);
      if (tr.dev) hipLaunchKernelGGL(k_mp_trace, dim3((unsigned)nblk), dim3(MP_TB), 0, ctx->stream, ncell, kmax, p, rd64, tr.dev);
      DZ_HIP(hipGetLastError());
      lap(4, t);
    }
  }
  std::vector<int> hflag(kmax);
  DZ_HIP(hipMemcpyAsync(hflag.data(), flags, (size_t)kmax * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = sp.finish()) || (rc = sn.finish()) || (rc = rd.finish()) || (rc = rs.finish()) || (rc = wd.finish()) || (rc = lk.finish()) ||
      (rc = rw.finish()) || (rc = tr.finish()))
    return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  int nf = 0;
  for (int p = 0; p < kmax; p++) nf += hflag[p] != 0;
  if (n_failed) *n_failed = nf;
  ctx->ksec.erase("map_post.lap");
  static const char *names[5] = {"map_post.gram", "map_post.factor", "map_post.inverse", "map_post.c", "map_post.rows"};
  double tot = 0.0;
  for (int i = 0; i < 5; i++) {
    ctx->ksec[names[i]] = sec[i];
    tot += sec[i];
  }
  ctx->ksec["map_posterior"] = tot;
  ctx->ksec["map_post.nb"] = MP_NB;
  ctx->ksec["map_post.mfma"] = mfma ? 1.0 : 0.0;
  return 0;
}
