// map_post_internal.h -- what map_post.hip (dazim_map_posterior, one dense block per period) and model_post.hip
// (dazim_model_posterior, one dense block for the whole 3-D model) share: the sizes of the dense kernels, their two tile forms, the
// fixed-order sum of a workgroup, and the host driver of the dense part (map_post_dense.hip), which both entries call -- so a block
// of the maps and the block of the model go through the same kernels in the same order, bit for bit.
#pragma once
#include "sparse_internal.h"

constexpr int MP_NB = 32;   // panel width of the factorisation and of the inverse (stat map_post.nb)
constexpr int MP_TS = 64;   // the tile kernels' output tile, MP_TS x MP_TS per workgroup of MP_TB threads
constexpr int MP_TB = 256;
constexpr int MP_LD = MP_TS + 1;

typedef double mp_v4 __attribute__((ext_vector_type(4)));

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

// the sums of a workgroup's MP_TB threads in a fixed order: butterfly inside a wavefront, the wavefronts' values in ascending order
__device__ __forceinline__ double mp_block_sum(double v, double *red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < MP_TB / 64; i++) s += red[i];
  return s;
}

#pragma GCC visibility push(hidden)
// The dense part on one block of ng unknowns, enqueued on the context's stream: Ad [ng][ng] holds the lower triangle of the normal
// matrix and ends as M = R^-1 (lower triangle), Cd [ng][max(ng, MP_NB)] is scratch for the inverse and ends as C = M^T M, both
// triangles; *flag (device) is set to 1 at a pivot that is not finite and > 0.  mfma: the tile form of the trailing update and of C.
// The seconds of factor, inverse and C are ADDED to sec[0..2]; they are measured with the context's events under the stat `lap`.
int dz_mp_dense(dazim_ctx *ctx, int ng, double *Ad, double *Cd, int *flag, bool mfma, const char *lap, double *sec);
#pragma GCC visibility pop
