// sparse_internal.h -- what sparse.hip (the matrix and its two products), lsmr.hip (the solver) and assemble.hip (generated rows,
// data weights, clamped updates) share: the CSR container, the reduction helpers of their kernels and the products' host side.
#pragma once
#include "dazim_internal.h"

struct dazim_csr {
  int64_t m = 0, n = 0, nnz = 0;
  int64_t *rowptr = nullptr, *colptr = nullptr;  // [m+1], [n+1]
  int *col = nullptr, *row = nullptr;            // CSR column / CSC row of each entry, 0-based
  float *val = nullptr, *tval = nullptr;         // CSR / CSC values
  unsigned *tperm = nullptr;                     // CSC entry -> CSR entry (for value rescaling)
  // column-blocked view of the (canonical: columns ascending inside a row) CSR for the scatter form
  // of A^T*y: row r's entries with column in block b are [cbptr[r*(ncb+1)+b], cbptr[r*(ncb+1)+b+1])
  int ncb = 0, cbw = 0;                          // number of column blocks, block width
  int64_t *cbptr = nullptr;
  float vmax = 0.0f;                             // max |val|, sets the fixed-point scale
  // rows [0, split_row) hold the long rows, the rows from split_row on are all shorter than SPLIT_SHORT entries (G: the ray rows,
  // then the seven-entry regularisation rows) -- the blocked products give each part the lane grouping it wants.  m: no short tail.
  int64_t split_row = 0;
  double long_avg = 0.0;                         // entries per row in [0, split_row)
  // the same column indices in 16 bits: the two products of an LSMR iteration stream 6 instead of 8 bytes per stored entry.
  // col16_mod = 0: the column itself (n <= 65536, the S-256 matrix); col16_mod = 2*cbw > 0: the column relative to the first
  // column of its PAIR of column blocks (larger n: the scatter kernel works on one block, the blocked A*x on a pair).
  // Built with the column blocks; nullptr when not used.
  unsigned short *col16 = nullptr;
  int64_t col16_cap = 0;                         // entries col16 can hold
  int col16_mod = 0;
  // rows / entries the arrays rowptr (cap_m + 1), col and val (cap_nnz) can hold: rays_build_G allocates them with the slack
  // the options csr.reserve_rows / csr.reserve_nnz ask for, so that the regularisation rows are appended in place
  // (0: exactly m / nnz)
  int64_t cap_m = 0, cap_nnz = 0;
  dazim_csr *twin = nullptr;   // option rays.dense_twin: the reference's dense copies GVs | GGc | GGs of the same rows
};

constexpr int WPB = 4;        // wavefronts per workgroup in the row kernels
constexpr int VB = 256;       // threads per block of the vector kernels
constexpr int NPART = 256;    // partial sums per reduction
constexpr int APART = 2048;   // partial maxima (enough workgroups to stream at HBM rate)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ void block_partial(double v, double *part) {
  __shared__ double s[VB / 64];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < VB / 64; i++) t += s[i];
    part[blockIdx.x] = t;
  }
}
inline int nblk(int64_t n, int cap = 2048) {
  int64_t b = (n + VB - 1) / VB;
  if (b < 1) b = 1;
  return (int)(b > cap ? cap : b);
}

// ---- host side of the products (sparse.hip), library-internal -----------------------------------------------------------------
#pragma GCC visibility push(hidden)
// workgroups of a row-kernel launch over nrows rows; nx = length of the gathered vector (< 0: not a product)
int dz_spmv_blocks(dazim_ctx *ctx, int64_t nrows, int64_t nx = -1);
bool dz_use_scatter(dazim_ctx *ctx, const dazim_csr *A);   // A^T*y takes the scatter form (no CSC copy needed)
// y(out, m) = beta*y + A x ; the number of ||out||^2 partials written to sumsq goes to *npart
int dz_launch_spmvA(dazim_ctx *ctx, const dazim_csr *A, const float *x, float *out, const float *beta_p, float beta_sign,
                    double *sumsq, int *npart, const int *guard = nullptr);
// x(out, n) = beta*x + A^T y, |y| <= ymax ; the number of ||out||^2 partials written to sumsq goes to *npart
int dz_launch_spmvT(dazim_ctx *ctx, const dazim_csr *A, const float *y, float ymax, float *out, const float *beta_p,
                    float beta_sign, double *sumsq, int *npart, const int *guard = nullptr);
// the CSC copy is only needed by the gather form of A^T*y: it is built on first use
int dz_build_transpose(dazim_ctx *ctx, dazim_csr *A);
int dz_invalidate_transpose(dazim_csr *A);
// column-block pointers + max|val| for the scatter form of A^T*y (needs canonical CSR)
// changed_from: first entry whose column index is new (0: all of them; < 0: only values changed, e.g. row scaling) -- the
// 16-bit copy of the column indices is extended / kept accordingly
int dz_build_colblocks(dazim_ctx *ctx, dazim_csr *A, int64_t changed_from = 0);
// rows [0, nrows) of A times w[row] (device); the CSC values and the fixed-point scale follow.  Synchronises the stream.
int dz_scale_rows(dazim_ctx *ctx, dazim_csr *A, int64_t nrows, const float *w);
#pragma GCC visibility pop
