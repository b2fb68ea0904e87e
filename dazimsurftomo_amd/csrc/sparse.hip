// sparse.hip -- K6 of SURVEY.md: the sensitivity matrix on the device (CSR + stable transpose + column blocks) and its two
// products (aprod, inv/aprod.f90:7).  The fp32 LSMR solver that runs on them is lsmr.hip; the generated regularisation rows, the
// data weights and the clamped updates are assemble.hip (both through sparse_internal.h).
//
// The products are HBM-bound: 8 B per stored entry (fp32 value + int32 index) are streamed once per
// product with 16-byte loads, one wavefront per row (CSR, A*x) or per column (CSC, A^T*y), and a
// 64-lane shuffle reduction; the gathered vector stays in L2.  Both products write their result in
// a fixed order (no atomics) so that LSMR is reproducible run to run.
#include "sparse_internal.h"

#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

// out[r] = beta*out[r] + sum_k val[k]*x[idx[k]], k in [ptr[r], ptr[r+1]) ; one wavefront per row.
// If sumsq != nullptr the workgroup also writes its partial sum of out[r]^2 (double) for a norm.
__global__ __launch_bounds__(64 * WPB) void spmv_rows(int64_t nrows, const int64_t *__restrict__ ptr,
                                                        const int *__restrict__ idx,
                                                        const float *__restrict__ val,
                                                        const float *__restrict__ x, float *__restrict__ out,
                                                        const float *__restrict__ beta_p, float beta_sign,
                                                        double *__restrict__ sumsq, const int *__restrict__ guard) {
  if (guard && *guard) return;   // LSMR has stopped (or skips this half-step): see LsmrState
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float beta = beta_p ? beta_sign * beta_p[0] : beta_sign;
  double sq = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * WPB + w; r < nrows; r += (int64_t)gridDim.x * WPB) {
    const int64_t s = ptr[r], e = ptr[r + 1];
    float acc = 0.0f;
    int64_t s4 = (s + 3) & ~(int64_t)3;
    if (s4 > e) s4 = e;
    for (int64_t i = s + lane; i < s4; i += 64) acc += val[i] * x[idx[i]];
    const int64_t e4 = s4 + ((e - s4) & ~(int64_t)3);
    for (int64_t i = s4 + 4 * lane; i < e4; i += 256) {
      const float4 v = *reinterpret_cast<const float4 *>(val + i);
      const int4 c = *reinterpret_cast<const int4 *>(idx + i);
      acc += v.x * x[c.x];
      acc += v.y * x[c.y];
      acc += v.z * x[c.z];
      acc += v.w * x[c.w];
    }
    for (int64_t i = e4 + lane; i < e; i += 64) acc += val[i] * x[idx[i]];
    acc = wave_sum(acc);
    if (lane == 0) {
      const float o = beta * out[r] + acc;
      out[r] = o;
      sq += (double)o * (double)o;
    }
  }
  if (sumsq) {
    __shared__ double s_sq[WPB];
    if (lane == 0) s_sq[w] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int i = 0; i < WPB; i++) t += s_sq[i];
      sumsq[blockIdx.x] = t;
    }
  }
}

// Same product with the dense vector staged in LDS: used when 4*len(x) fits (<= 152 KB), which
// removes the per-entry cache-line gather that otherwise bounds the product (~1 line/clk/CU).
// One workgroup of 16 wavefronts per CU, each wavefront a row at a time, two 16-byte loads of
// values and of indices in flight per lane.
constexpr int LWPB = 16;
// four consecutive column indices with one load: int4 (16 bytes) or ushort4 (8 bytes)
template <class IT> struct Idx4;
template <> struct Idx4<int> { using type = int4; };
template <> struct Idx4<unsigned short> { using type = ushort4; };
template <class IT>
__global__ __launch_bounds__(64 * LWPB) void spmv_rows_ldsx(int64_t nrows, int64_t nx, const int64_t *__restrict__ ptr,
                                                           const IT *__restrict__ idx, const float *__restrict__ val,
                                                           const float *__restrict__ x, float *__restrict__ out,
                                                           const float *__restrict__ beta_p, float beta_sign,
                                                           double *__restrict__ sumsq, const int *__restrict__ guard) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  if (guard && *guard) return;
  for (int64_t i = threadIdx.x * 4; i < nx; i += 64 * LWPB * 4) {
    if (i + 3 < nx)
      *reinterpret_cast<float4 *>(xs + i) = *reinterpret_cast<const float4 *>(x + i);
    else
      for (int64_t j = i; j < nx; j++) xs[j] = x[j];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float beta = beta_p ? beta_sign * beta_p[0] : beta_sign;
  double sq = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * LWPB + w; r < nrows; r += (int64_t)gridDim.x * LWPB) {
    const int64_t s = ptr[r], e = ptr[r + 1];
    float acc = 0.0f;
    int64_t s4 = (s + 3) & ~(int64_t)3;
    if (s4 > e) s4 = e;
    for (int64_t i = s + lane; i < s4; i += 64) acc += val[i] * xs[idx[i]];
    const int64_t e4 = s4 + ((e - s4) & ~(int64_t)3);
    int64_t i = s4 + 4 * lane;
    for (; i + 768 < e4; i += 1024) {   // four groups in flight (16-bit indices leave 24 instead of 32 bytes per lane and group)
      using I4 = typename Idx4<IT>::type;
      float4 v[4];
      I4 c[4];
#pragma unroll
      for (int g = 0; g < 4; g++) {
        v[g] = *reinterpret_cast<const float4 *>(val + i + 256 * g);
        c[g] = *reinterpret_cast<const I4 *>(idx + i + 256 * g);
      }
#pragma unroll
      for (int g = 0; g < 4; g++) {
        acc += v[g].x * xs[c[g].x];
        acc += v[g].y * xs[c[g].y];
        acc += v[g].z * xs[c[g].z];
        acc += v[g].w * xs[c[g].w];
      }
    }
    for (; i + 256 < e4; i += 512) {
      using I4 = typename Idx4<IT>::type;
      const float4 v0 = *reinterpret_cast<const float4 *>(val + i);
      const I4 c0 = *reinterpret_cast<const I4 *>(idx + i);
      const float4 v1 = *reinterpret_cast<const float4 *>(val + i + 256);
      const I4 c1 = *reinterpret_cast<const I4 *>(idx + i + 256);
      acc += v0.x * xs[c0.x];
      acc += v0.y * xs[c0.y];
      acc += v0.z * xs[c0.z];
      acc += v0.w * xs[c0.w];
      acc += v1.x * xs[c1.x];
      acc += v1.y * xs[c1.y];
      acc += v1.z * xs[c1.z];
      acc += v1.w * xs[c1.w];
    }
    for (; i < e4; i += 256) {
      using I4 = typename Idx4<IT>::type;
      const float4 v = *reinterpret_cast<const float4 *>(val + i);
      const I4 c = *reinterpret_cast<const I4 *>(idx + i);
      acc += v.x * xs[c.x];
      acc += v.y * xs[c.y];
      acc += v.z * xs[c.z];
      acc += v.w * xs[c.w];
    }
    for (int64_t k = e4 + lane; k < e; k += 64) acc += val[k] * xs[idx[k]];
    acc = wave_sum(acc);
    if (lane == 0) {
      const float o = beta * out[r] + acc;
      out[r] = o;
      sq += (double)o * (double)o;
    }
  }
  if (sumsq) {
    __shared__ double s_sq[LWPB];
    if (lane == 0) s_sq[w] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int k = 0; k < LWPB; k++) t += s_sq[k];
      sumsq[blockIdx.x] = t;
    }
  }
}
__global__ void k_scale_rows(int64_t nrows, const int64_t *ptr, float *val, const float *w) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * WPB + wv; r < nrows; r += (int64_t)gridDim.x * WPB) {
    const float a = w[r];
    for (int64_t i = ptr[r] + lane; i < ptr[r + 1]; i += 64) val[i] *= a;
  }
}
// out[col[i]] += |val[i]|: the reference's DWS, norm(col(i))=norm(col(i))+abs(rw(i)), inv/Main_Jt.f90:477-481
// Accumulated in 64-bit fixed point (integer addition is associative: the result does not depend on the order in which the
// atomics land, so DWS is reproducible run to run), then converted.
__global__ void k_col_abs_sums(int64_t n, const int *col, const float *val, double scale, unsigned long long *acc) {
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
    atomicAdd(&acc[col[i]], (unsigned long long)__double2ll_rn((double)fabsf(val[i]) * scale));
}
__global__ void k_fixed_to_float(int64_t n, const unsigned long long *acc, double inv_scale, float *out) {
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) out[i] = (float)((double)acc[i] * inv_scale);
}
__global__ void k_gather_f(int64_t n, const unsigned *perm, const float *src, float *dst) {
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) dst[i] = src[perm[i]];
}
__global__ void k_gather_i(int64_t n, const unsigned *perm, const int *src, int *dst, int add) {
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) dst[i] = src[perm ? perm[i] : (unsigned)i] + add;
}
__global__ void k_iota_keys(int64_t n, const int *one_based, unsigned *keys, unsigned *iota) {
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) {
    if (keys) keys[i] = (unsigned)(one_based[i] - 1);
    iota[i] = (unsigned)i;
  }
}
// ptr[r] = first position in the sorted key array whose key >= r  (r = 0..nrows)
__global__ void k_lower_bound(int64_t nrows, int64_t nnz, const unsigned *keys, int64_t *ptr) {
  for (int64_t r = (int64_t)blockIdx.x * VB + threadIdx.x; r <= nrows; r += (int64_t)gridDim.x * VB) {
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)keys[mid] < r) lo = mid + 1; else hi = mid;
    }
    ptr[r] = lo;
  }
}
__global__ void k_check_range(int64_t n, const int *a, int lo, int hi, int *bad) {
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
    if (a[i] < lo || a[i] > hi) atomicOr(bad, 1);
}

// ---- A^T*y in scatter form ---------------------------------------------------------------------
// The gather form (one wavefront per CSC column) is bound by one cache-line fetch of y per entry.
// The scatter form streams the CSR rows instead -- y[r] is a per-row scalar, no gather at all -- and
// accumulates val*y[r] into per-column accumulators in LDS.  To stay reproducible the accumulators
// are 64-bit fixed point (integer addition is associative, so the order in which wavefronts arrive
// does not matter; the quantum is 2^-40 of the largest |val*y|, far below fp32 round-off).  Columns
// are split into blocks that fit LDS; a workgroup owns (row chunk, column block) and per-chunk
// partials are combined in a second, equally order-free, pass.
constexpr int SCW = 16;             // wavefronts per workgroup
constexpr int CBW_MAX = 19 * 1024;  // int64 accumulators per column block (152 KB)

__global__ void k_colblock_ptr(int64_t nrows, int ncb, int cbw, const int64_t *__restrict__ ptr,
                               const int *__restrict__ col, int64_t *__restrict__ cbptr) {
  const int64_t t = (int64_t)blockIdx.x * VB + threadIdx.x;
  if (t >= nrows * (ncb + 1)) return;
  const int64_t r = t / (ncb + 1);
  const int b = (int)(t - r * (ncb + 1));
  int64_t lo = ptr[r], hi = ptr[r + 1];
  const int target = b * cbw;  // first entry with col >= target
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col[mid] < target) lo = mid + 1; else hi = mid;
  }
  cbptr[t] = lo;
}
// 1 + the last row with at least `thresh` entries (0: none): behind it the matrix has only short rows
constexpr int SPLIT_SHORT = 64;
__global__ void k_last_long_row(int64_t nrows, const int64_t *__restrict__ ptr, int thresh, unsigned long long *res) {
  unsigned long long best = 0;
  for (int64_t r = (int64_t)blockIdx.x * VB + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * VB)
    if (ptr[r + 1] - ptr[r] >= thresh) best = (unsigned long long)(r + 1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long b = __shfl_xor(best, o);
    best = b > best ? b : best;
  }
  if ((threadIdx.x & 63) == 0 && best) atomicMax(res, best);
}
// 32-bit -> 16-bit column indices, four per thread step; mod > 0: relative to the pair of column blocks (column mod 2*cbw)
__global__ void k_narrow_cols(int64_t n, const int *__restrict__ col, unsigned short *__restrict__ col16, int mod) {
  for (int64_t i = ((int64_t)blockIdx.x * VB + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * VB * 4) {
    if (i + 3 < n) {
      int4 c = *reinterpret_cast<const int4 *>(col + i);
      if (mod > 0) { c.x %= mod; c.y %= mod; c.z %= mod; c.w %= mod; }
      *reinterpret_cast<ushort4 *>(col16 + i) = make_ushort4((unsigned short)c.x, (unsigned short)c.y, (unsigned short)c.z, (unsigned short)c.w);
    } else {
      for (int64_t j = i; j < n; j++) col16[j] = (unsigned short)(mod > 0 ? col[j] % mod : col[j]);
    }
  }
}
// max |x| over the bit patterns of |x| as unsigned integers: they order like the values for finite x, Inf above every finite
// value and NaN above Inf, so a NaN anywhere in x is the result (fmaxf would drop it) and an Inf is the result unless a NaN is
__device__ __forceinline__ unsigned abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ unsigned umax2(unsigned a, unsigned b) { return a > b ? a : b; }
__global__ void k_absmax(int64_t n, const float *x, float *part) {
  unsigned v = 0u;
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? n / 4 : 0;   // 16-byte loads when the array allows
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * VB) {
    const float4 q = reinterpret_cast<const float4 *>(x)[i];
    v = umax2(umax2(v, umax2(abs_bits(q.x), abs_bits(q.y))), umax2(abs_bits(q.z), abs_bits(q.w)));
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) v = umax2(v, abs_bits(x[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umax2(v, (unsigned)__shfl_xor((int)v, o));
  __shared__ unsigned s[VB / 64];
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0u;
    for (int i = 0; i < VB / 64; i++) t = umax2(t, s[i]);
    part[blockIdx.x] = __uint_as_float(t);
  }
}
__global__ void k_absmax_finish(const float *part, int np, float *res) {
  unsigned v = 0u;
  for (int i = threadIdx.x; i < np; i += 64) v = umax2(v, abs_bits(part[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umax2(v, (unsigned)__shfl_xor((int)v, o));
  if (threadIdx.x == 0) res[0] = __uint_as_float(v);
}

// ---- software-pipelined walk over CSR row segments (A^T*y scatter and column-blocked A*x) ----
// These kernels are bound by the dependent loads of a row (its pointers -> its entries -> the arithmetic), not by bandwidth, so
// each lane group keeps three rows in flight: while the entries of row i are consumed, those of row i+1 are arriving and the
// pointers of row i+2 are requested.  All prefetch loads are unconditional (a lane with nothing to fetch reads entry 0), so that
// the compiler can count them and wait only for the oldest ones; rows with more than 4*NG*GL aligned entries finish in a plain
// loop.  GL = lanes that share one row (64, or 16 for short segments: four rows per wavefront at a time); rows r_first,
// r_first + stride, ... below nrows are visited; ptrf(r) -> {s, e, aux} gives the entry range and one per-row float,
// elemf(column, value, aux) is called for every entry (head, aligned groups, tail: the order of a plain loop over this lane's
// entries), endf(r, aux) once per row.
struct RowPtr { int64_t s, e; float aux; };
template <int GL, int NG, class IT, class PtrF, class ElemF, class EndF>
__device__ __forceinline__ void walk_rows(int64_t r_first, int64_t stride, int64_t nrows, int lane, const IT *__restrict__ col,
                                          const float *__restrict__ val, PtrF ptrf, ElemF elemf, EndF endf) {
  using I4 = typename Idx4<IT>::type;
  struct Ent { int64_t r, s4, e4; float aux; float4 v[NG]; I4 k[NG]; float hv, tv; int hk, tk; bool hh, ht; };
  auto load_ptr = [&](int64_t r) {
    RowPtr p = ptrf(r < nrows ? r : 0);                // (a dummy read past the end)
    if (r >= nrows) p.e = p.s;                         // nothing to do
    return p;
  };
  auto issue = [&](int64_t r, const RowPtr &p) {
    Ent t;
    t.r = r;
    t.aux = p.aux;
    t.s4 = (p.s + 3) & ~(int64_t)3;
    if (t.s4 > p.e) t.s4 = p.e;
    t.e4 = t.s4 + ((p.e - t.s4) & ~(int64_t)3);
#pragma unroll
    for (int g = 0; g < NG; g++) {
      const int64_t i = t.s4 + 4 * lane + (int64_t)g * 4 * GL;
      const int64_t j = i < t.e4 ? i : 0;
      t.v[g] = *reinterpret_cast<const float4 *>(val + j);
      t.k[g] = *reinterpret_cast<const I4 *>(col + j);
    }
    const int64_t ih = p.s + lane, it = t.e4 + lane;   // <= 3 unaligned entries at either end
    t.hh = ih < t.s4;
    t.ht = it < p.e;
    t.hv = val[t.hh ? ih : 0];
    t.hk = (int)col[t.hh ? ih : 0];
    t.tv = val[t.ht ? it : 0];
    t.tk = (int)col[t.ht ? it : 0];
    return t;
  };
  auto consume = [&](const Ent &t) {
    if (t.hh) elemf(t.hk, t.hv, t.aux);
#pragma unroll
    for (int g = 0; g < NG; g++) {
      const int64_t i = t.s4 + 4 * lane + (int64_t)g * 4 * GL;
      if (i < t.e4) {
        elemf((int)t.k[g].x, t.v[g].x, t.aux); elemf((int)t.k[g].y, t.v[g].y, t.aux);
        elemf((int)t.k[g].z, t.v[g].z, t.aux); elemf((int)t.k[g].w, t.v[g].w, t.aux);
      }
    }
    for (int64_t i = t.s4 + 4 * lane + (int64_t)NG * 4 * GL; i < t.e4; i += 4 * GL) {   // long rows
      const float4 v = *reinterpret_cast<const float4 *>(val + i);
      const I4 k = *reinterpret_cast<const I4 *>(col + i);
      elemf((int)k.x, v.x, t.aux); elemf((int)k.y, v.y, t.aux); elemf((int)k.z, v.z, t.aux); elemf((int)k.w, v.w, t.aux);
    }
    if (t.ht) elemf(t.tk, t.tv, t.aux);
    endf(t.r, t.aux);
  };
  int64_t r = r_first;
  Ent eC = issue(r, load_ptr(r));
  RowPtr pB = load_ptr(r + stride);
  for (; r < nrows; r += stride) {   // (rows differ per 16-lane group when GL = 16: the groups simply diverge at the end)
    const RowPtr pA = load_ptr(r + 2 * stride);
    const Ent eB = issue(r + stride, pB);
    consume(eC);
    eC = eB;
    pB = pA;
  }
}

// A^T*y: GL lanes share one (row, column block) segment and walk it with walk_rows.
// Row steps are dealt round-robin over all wavefronts of the launch (step k goes to workgroup k mod nchunk): G's ray rows hold
// hundreds to thousands of entries and its Tikhonov rows seven, so contiguous chunks of equal rows or equal entries leave CUs
// idle, while a counter that hands rows out dynamically costs more in same-address atomics than it saves (both measured).
// (The same pipeline applied to the LDS-staged A*x kernel made it 2 % slower -- that kernel streams whole rows and is bandwidth
// bound already -- and pipelining fixed-size segments instead of rows made this one 6 % slower; same-box A/B runs.)
template <int GL, int NG, class IT>
__global__ __launch_bounds__(64 * SCW) void spmvT_scatter(int64_t nsplit, int64_t nrows, int nchunk, int ncb, int cbw, int64_t ncols,
                                                          const int64_t *__restrict__ cbptr, const IT *__restrict__ col,
                                                          const float *__restrict__ val, const float *__restrict__ y,
                                                          double scale, long long *__restrict__ part, const int *__restrict__ guard,
                                                          int pairlocal) {
  extern __shared__ __attribute__((aligned(16))) long long acc[];
  if (guard && *guard) return;
  const int chunk = blockIdx.x / ncb, cb = blockIdx.x - chunk * ncb;
  const int c0 = cb * cbw;
  const int csub = pairlocal ? (cb & 1) * cbw : c0;    // what to take off a stored index to get the accumulator
  const int width = (int)((ncols - c0) < cbw ? (ncols - c0) : cbw);
  for (int i = threadIdx.x; i < width; i += 64 * SCW) acc[i] = 0;
  __syncthreads();
  constexpr int RPWV = 64 / GL;                        // rows per wavefront and step
  const int lane = (threadIdx.x & 63) % GL, grp = (threadIdx.x & 63) / GL;
  // fixed point by the magic-number trick: for |t| < 2^51, the low mantissa bits of t + 1.5*2^52 hold round-to-nearest-even(t);
  // scale is a power of two, so the fused multiply-add rounds exactly like (v*y*scale) + magic would
  constexpr double MAGIC = 6755399441055744.0;
  // (two walks, round 5: the long rows [0, nsplit) with GL lanes per row, the short tail [nsplit, nrows) -- G's seven-entry
  // regularisation rows behind its ray rows -- four rows per wavefront; one launch, one set of accumulators)
  auto ptrf = [&](int64_t r) { return RowPtr{cbptr[r * (ncb + 1) + cb], cbptr[r * (ncb + 1) + cb + 1], y[r]}; };
  auto elemf = [&](int c, float v, float yr) {
    atomicAdd((unsigned long long *)&acc[c - csub],
              (unsigned long long)(__double_as_longlong(fma((double)(v * yr), scale, MAGIC)) - __double_as_longlong(MAGIC)));
  };
  // (contiguous row ranges of equal entry counts per wavefront instead of this round-robin deal were measured in round 5: A*x 83 ->
  // 108 us, A^T*y 103 -> 135 us on test4_Yunnan's system -- dealt round-robin, the wavefronts of the launch stream one moving
  // window of the matrix together, which the memory system likes better than 2 048 separate streams)
  walk_rows<GL, NG, IT>(((int64_t)chunk + (int64_t)nchunk * (threadIdx.x >> 6)) * RPWV + grp, (int64_t)nchunk * SCW * RPWV, nsplit, lane,
                        col, val, ptrf, elemf, [](int64_t, float) {});
  if (nsplit < nrows) {
    constexpr int GS = 16, RS = 64 / GS;
    const int lane_s = (threadIdx.x & 63) % GS, grp_s = (threadIdx.x & 63) / GS;
    walk_rows<GS, 1, IT>(nsplit + ((int64_t)chunk + (int64_t)nchunk * (threadIdx.x >> 6)) * RS + grp_s, (int64_t)nchunk * SCW * RS, nrows,
                         lane_s, col, val, ptrf, elemf, [](int64_t, float) {});
  }
  __syncthreads();
  long long *dst = part + (size_t)chunk * ncols + c0;
  for (int i = threadIdx.x; i < width; i += 64 * SCW) dst[i] = acc[i];
}
// out[c] = beta*out[c] + sum_chunks part[chunk][c] / scale ; partial ||out||^2
__global__ void k_scatter_combine(int64_t ncols, int nchunk, const long long *__restrict__ part, double inv_scale,
                                  float *__restrict__ out, const float *__restrict__ beta_p, float beta_sign,
                                  double *__restrict__ sumsq, const int *__restrict__ guard) {
  if (guard && *guard) return;
  const float beta = beta_p ? beta_sign * beta_p[0] : beta_sign;
  double sq = 0.0;
  for (int64_t c = (int64_t)blockIdx.x * VB + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * VB) {
    // eight independent partial sums: the loads of a column are in flight together (integer sums: any order gives the same bits)
    long long t8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int k = 0;
    for (; k + 8 <= nchunk; k += 8)
#pragma unroll
      for (int j = 0; j < 8; j++) t8[j] += part[(size_t)(k + j) * ncols + c];
    for (; k < nchunk; k++) t8[0] += part[(size_t)k * ncols + c];
    const long long t = ((t8[0] + t8[1]) + (t8[2] + t8[3])) + ((t8[4] + t8[5]) + (t8[6] + t8[7]));
    const float o = beta * out[c] + (float)((double)t * inv_scale);
    out[c] = o;
    sq += (double)o * o;
  }
  if (sumsq) block_partial(sq, sumsq);
}

// A*x for matrices whose x does not fit the LDS (n > 38 K: joint inversions, S-512): the columns are cut at the same block
// pointers as the scatter kernel, two scatter blocks (<= 38 K floats of x) per workgroup, which removes the per-entry
// cache-line gather that bounds the plain kernel.  A workgroup owns (row set x column-block pair) and writes the partial
// dot product of each of its rows to part[pair][row]; k_rows_combine adds the pairs in a fixed order.
template <int GL, int NG, class IT>
__global__ __launch_bounds__(64 * SCW) void spmv_rows_blocked(int64_t nsplit, int64_t nrows, int nset, int npair, int ncb, int cbw, int64_t ncols,
                                                              const int64_t *__restrict__ cbptr, const IT *__restrict__ col,
                                                              const float *__restrict__ val, const float *__restrict__ x,
                                                              float *__restrict__ part, const int *__restrict__ guard, int pairlocal) {
  extern __shared__ __attribute__((aligned(16))) float xblk[];
  if (guard && *guard) return;
  const int set = blockIdx.x / npair, pr = blockIdx.x - set * npair;
  const int cb0 = 2 * pr, cb1 = (cb0 + 2 < ncb) ? cb0 + 2 : ncb;
  const int c0 = cb0 * cbw;
  const int csub = pairlocal ? 0 : c0;                 // (16-bit indices of large matrices are already relative to the pair)
  const int width = (int)((ncols - c0) < 2 * (int64_t)cbw ? (ncols - c0) : 2 * (int64_t)cbw);
  for (int i = threadIdx.x; i < width; i += 64 * SCW) xblk[i] = x[c0 + i];
  __syncthreads();
  constexpr int RPWV = 64 / GL;
  const int lane = (threadIdx.x & 63) % GL, grp = (threadIdx.x & 63) / GL;
  float acc = 0.0f;
  float *dst = part + (size_t)pr * nrows;
  auto ptrf = [&](int64_t r) { return RowPtr{cbptr[r * (ncb + 1) + cb0], cbptr[r * (ncb + 1) + cb1], 0.0f}; };
  auto elemf = [&](int c, float v, float) { acc += v * xblk[c - csub]; };
  walk_rows<GL, NG, IT>(((int64_t)set + (int64_t)nset * (threadIdx.x >> 6)) * RPWV + grp, (int64_t)nset * SCW * RPWV, nsplit, lane, col, val,
                        ptrf, elemf, [&](int64_t r, float) {
                          float a = acc;
#pragma unroll
                          for (int o = GL / 2; o > 0; o >>= 1) a += __shfl_xor(a, o);
                          if (lane == 0 && r < nsplit) dst[r] = a;
                          acc = 0.0f;
                        });
  if (nsplit < nrows) {   // the short tail of the matrix (see spmvT_scatter): four rows per wavefront
    constexpr int GS = 16, RS = 64 / GS;
    const int lane_s = (threadIdx.x & 63) % GS, grp_s = (threadIdx.x & 63) / GS;
    acc = 0.0f;
    walk_rows<GS, 1, IT>(nsplit + ((int64_t)set + (int64_t)nset * (threadIdx.x >> 6)) * RS + grp_s, (int64_t)nset * SCW * RS, nrows, lane_s,
                         col, val, ptrf, elemf, [&](int64_t r, float) {
                           float a = acc;
#pragma unroll
                           for (int o = GS / 2; o > 0; o >>= 1) a += __shfl_xor(a, o);
                           if (lane_s == 0 && r < nrows) dst[r] = a;
                           acc = 0.0f;
                         });
  }
}
// out[r] = beta*out[r] + sum_pairs part[pair][r] ; partial ||out||^2
__global__ void k_rows_combine(int64_t nrows, int npair, const float *__restrict__ part, float *__restrict__ out,
                               const float *__restrict__ beta_p, float beta_sign, double *__restrict__ sumsq,
                               const int *__restrict__ guard) {
  if (guard && *guard) return;
  const float beta = beta_p ? beta_sign * beta_p[0] : beta_sign;
  double sq = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
    float t = part[r];
    for (int k = 1; k < npair; k++) t += part[(size_t)k * nrows + r];
    const float o = beta * out[r] + t;
    out[r] = o;
    sq += (double)o * o;
  }
  if (sumsq) block_partial(sq, sumsq);
}

constexpr int64_t LDSX_MAX = 38 * 1024;  // floats of the dense vector that fit the 160 KB LDS next to the reduction scratch
bool use_ldsx(dazim_ctx *ctx, int64_t nrows, int64_t nx) {
  if (dz_opt(ctx, "spmv.ldsx", 1) == 0) return false;
  return nx <= LDSX_MAX && nrows >= (int64_t)ctx->num_cu * LWPB * 4;
}
// nx = length of the gathered vector; nblocks must come from dz_spmv_blocks(ctx, nrows, nx)
int launch_spmv(dazim_ctx *ctx, int64_t nrows, int64_t nx, const int64_t *ptr, const int *idx, const float *val,
                const float *x, float *out, const float *beta_p, float beta_sign, double *sumsq,
                int nblocks, const int *guard = nullptr, const unsigned short *idx16 = nullptr) {
  if (use_ldsx(ctx, nrows, nx)) {
    const size_t lds = (size_t)((nx + 3) & ~(int64_t)3) * 4;
    if (idx16) {   // 16-bit column indices: 6 bytes per stored entry
      DZ_HIP(hipFuncSetAttribute((const void *)spmv_rows_ldsx<unsigned short>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(spmv_rows_ldsx<unsigned short>, dim3(nblocks), dim3(64 * LWPB), lds, ctx->stream, nrows, nx, ptr, idx16, val,
                         x, out, beta_p, beta_sign, sumsq, guard);
    } else {
      DZ_HIP(hipFuncSetAttribute((const void *)spmv_rows_ldsx<int>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(spmv_rows_ldsx<int>, dim3(nblocks), dim3(64 * LWPB), lds, ctx->stream, nrows, nx, ptr, idx, val, x, out,
                         beta_p, beta_sign, sumsq, guard);
    }
  } else {
    hipLaunchKernelGGL(spmv_rows, dim3(nblocks), dim3(64 * WPB), 0, ctx->stream, nrows, ptr, idx, val, x, out,
                       beta_p, beta_sign, sumsq, guard);
  }
  DZ_HIP(hipGetLastError());
  return 0;
}
// row id of every CSR entry (one wavefront per row)
__global__ void k_expand_rows(int64_t nrows, const int64_t *ptr, unsigned *rowid) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * WPB + wv; r < nrows; r += (int64_t)gridDim.x * WPB)
    for (int64_t i = ptr[r] + lane; i < ptr[r + 1]; i += 64) rowid[i] = (unsigned)r;
}
__global__ void k_offset_ptr(int64_t n, const int64_t *src, int64_t add, int64_t *dst) {
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB) dst[i] = src[i] + add;
}
// dazim_csr_threshold: one wavefront per row; entries with |val| > tol keep their order (ballot prefix)
template <bool FILL>
__global__ __launch_bounds__(256) void k_threshold_rows(int64_t m, const int64_t *__restrict__ rowptr, const int *__restrict__ col,
                                                        const float *__restrict__ val, float tol, long *__restrict__ cnt,
                                                        const long *__restrict__ rowptr2, int *__restrict__ col2,
                                                        float *__restrict__ val2) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r > m) return;
  if (r == m) {
    if (!FILL && lane == 0) cnt[m] = 0;
    return;
  }
  const int64_t s = rowptr[r], e = rowptr[r + 1];
  long kept = 0;
  const long o = FILL ? rowptr2[r] : 0;
  for (int64_t i = s; i < e; i += 64) {
    const int64_t k = i + lane;
    float v = 0.0f;
    int c = 0;
    if (k < e) { v = val[k]; c = col[k]; }
    const bool keep = k < e && fabsf(v) > tol;
    const unsigned long long b = __ballot(keep);
    if (FILL && keep) {
      const long q = o + kept + __popcll(b & ((1ull << lane) - 1ull));
      val2[q] = v;
      col2[q] = c;
    }
    kept += __popcll(b);
  }
  if (!FILL && lane == 0) cnt[r] = kept;
}

bool use_blocked(dazim_ctx *ctx, const dazim_csr *A) {
  if (dz_opt(ctx, "spmv.blocked", 1) == 0) return false;
  return A->cbptr && A->n > LDSX_MAX && A->nnz >= (1 << 22) && A->m >= (int64_t)ctx->num_cu * SCW;
}
// *res = max |x[0..n)| of a device vector: enqueued, valid after the next synchronisation of the stream
int absmax_to_host(dazim_ctx *ctx, const float *x, int64_t n, float *res) {
  int rc;
  float *pm;
  if ((rc = dz_scratch(ctx, "csr.absmax", (size_t)APART + 4, &pm))) return rc;
  const int nb = nblk((n + 3) / 4, APART);
  hipLaunchKernelGGL(k_absmax, dim3(nb), dim3(VB), 0, ctx->stream, n, x, pm);
  hipLaunchKernelGGL(k_absmax_finish, dim3(1), dim3(64), 0, ctx->stream, pm, nb, pm + APART);
  DZ_HIP(hipMemcpyAsync(res, pm + APART, 4, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}
// the power of two that puts terms of magnitude <= pm on the 64-bit fixed-point grid of a sum over at most m rows
double fixed_scale(double pm, int64_t m) {
  int e = 0;
  if (pm > 0) (void)frexp(pm, &e);   // pm = f * 2^e, 0.5 <= f < 1  ->  pm < 2^e
  // fractional bits: every term is below 2^fb in fixed point and a column holds at most m of them, so the int64 sum needs
  // fb + ceil(log2 m) <= 62.  40 bits up to 4 M rows (quantum 2^-40 of the largest term), fewer beyond (still < fp32 round-off)
  int lgm = 0;
  while (((int64_t)1 << lgm) < m) lgm++;
  const int fb = 62 - lgm < 40 ? 62 - lgm : 40;
  return ldexp(1.0, fb - e);
}
// How the two blocked products walk the rows: [0, nsplit) with a lane group per (row, column block) segment, the short tail
// [nsplit, m) four rows per wavefront (option spmv.split = 0: no tail).  shortseg: the segments of the LONG rows hold fewer
// entries than `thresh` per row on average, so four rows per wavefront (16 lanes each) serve them too, else a whole wavefront
// per row -- test4_Yunnan's joint matrix is 20 877 ray rows of 2 548 entries and 73 440 regularisation rows of seven, 284 per
// segment on average, 637 in the ray rows
struct RowSplit { int64_t nsplit; bool shortseg; };
RowSplit row_split(dazim_ctx *ctx, const dazim_csr *A, double thresh) {
  const bool split = dz_opt(ctx, "spmv.split", 1) != 0 && A->split_row < A->m;
  return {split ? A->split_row : A->m, (split ? A->long_avg : (double)A->nnz / (double)A->m) < thresh};
}
// launch(GL, NG, column array) with the <GL, NG, IT> of a walk_rows kernel: 16 lanes and two groups in flight per row segment for
// short segments, 64 and four else; the 16-bit column indices (6 bytes per stored entry) where the matrix has them.  These four
// are the only instantiations of either kernel.
// (more or fewer 256-entry groups in flight per row segment -- 3 or 6 instead of 4 -- measured in round 5: no difference)
template <class F>
int dispatch_rows(const dazim_csr *A, bool shortseg, F launch) {
  using GL16 = std::integral_constant<int, 16>; using NG2 = std::integral_constant<int, 2>;
  using GL64 = std::integral_constant<int, 64>; using NG4 = std::integral_constant<int, 4>;
  if (A->col16) return shortseg ? launch(GL16(), NG2(), A->col16) : launch(GL64(), NG4(), A->col16);
  return shortseg ? launch(GL16(), NG2(), A->col) : launch(GL64(), NG4(), A->col);
}

}  // namespace

int dz_spmv_blocks(dazim_ctx *ctx, int64_t nrows, int64_t nx) {
  if (nx >= 0 && use_ldsx(ctx, nrows, nx)) return ctx->num_cu;  // one 16-wave workgroup per CU
  int64_t b = (nrows + WPB - 1) / WPB;
  const int64_t cap = (int64_t)ctx->num_cu * 8;  // 8 workgroups (32 waves) per CU, grid-stride the rest
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

int dz_invalidate_transpose(dazim_csr *A) {
  for (void **pp : {(void **)&A->colptr, (void **)&A->row, (void **)&A->tval, (void **)&A->tperm})
    if (*pp) { (void)hipFree(*pp); *pp = nullptr; }
  return 0;
}
// build the stable transpose (colptr,row,tval,tperm) of A's CSR arrays
int dz_build_transpose(dazim_ctx *ctx, dazim_csr *A) {
  const int64_t nnz = A->nnz, n = A->n, m = A->m;
  const size_t nz = (size_t)(nnz > 0 ? nnz : 1);
  (void)dz_invalidate_transpose(A);
  DZ_HIP(dz_malloc_retry(ctx, (void **)&A->colptr, (n + 1) * 8));
  DZ_HIP(dz_malloc_retry(ctx, (void **)&A->row, nz * 4));
  DZ_HIP(dz_malloc_retry(ctx, (void **)&A->tval, nz * 4));
  DZ_HIP(dz_malloc_retry(ctx, (void **)&A->tperm, nz * 4));
  if (nnz == 0) {
    DZ_HIP(hipMemsetAsync(A->colptr, 0, (n + 1) * 8, ctx->stream));
    return 0;
  }
  int rc;
  unsigned *ck, *cks, *iota, *rowid;
  if ((rc = dz_scratch(ctx, "csr.k0", nz, &ck)) || (rc = dz_scratch(ctx, "csr.k1", nz, &cks)) ||
      (rc = dz_scratch(ctx, "csr.v0", nz, &iota)) || (rc = dz_scratch(ctx, "csr.perm", nz, &rowid)))
    return rc;
  const int nb = nblk(nnz);
  int cbits = 1;
  while (((int64_t)1 << cbits) < n) cbits++;
  // keys = column (0-based) + 1 so that k_iota_keys' "-1" applies
  hipLaunchKernelGGL(k_gather_i, dim3(nb), dim3(VB), 0, ctx->stream, nnz, (const unsigned *)nullptr, A->col, (int *)ck, 0);
  hipLaunchKernelGGL(k_iota_keys, dim3(nb), dim3(VB), 0, ctx->stream, nnz, (const int *)nullptr, (unsigned *)nullptr, iota);
  hipLaunchKernelGGL(k_expand_rows, dim3(dz_spmv_blocks(ctx, m, -1)), dim3(64 * WPB), 0, ctx->stream, m, A->rowptr, rowid);
  size_t tb = 0;
  DZ_HIP(rocprim::radix_sort_pairs(nullptr, tb, ck, cks, iota, A->tperm, (size_t)nnz, 0, cbits, ctx->stream));
  void *tmp;
  if ((rc = dz_scratch(ctx, "csr.tmp", tb + 256, &tmp))) return rc;
  DZ_HIP(rocprim::radix_sort_pairs(tmp, tb, ck, cks, iota, A->tperm, (size_t)nnz, 0, cbits, ctx->stream));
  hipLaunchKernelGGL(k_lower_bound, dim3(nblk(n + 1)), dim3(VB), 0, ctx->stream, n, nnz, cks, A->colptr);
  hipLaunchKernelGGL(k_gather_f, dim3(nb), dim3(VB), 0, ctx->stream, nnz, A->tperm, A->val, A->tval);
  hipLaunchKernelGGL(k_gather_i, dim3(nb), dim3(VB), 0, ctx->stream, nnz, A->tperm, (const int *)rowid, A->row, 0);
  DZ_HIP(hipGetLastError());
  return 0;
}

int dz_build_colblocks(dazim_ctx *ctx, dazim_csr *A, int64_t changed_from) {
  if (A->cbptr) { dz_big_put(ctx, A->cbptr); A->cbptr = nullptr; }
  A->ncb = (int)((A->n + CBW_MAX - 1) / CBW_MAX);
  A->cbw = (int)(((A->n + A->ncb - 1) / A->ncb + 3) & ~3ll);
  const int mod16 = A->n <= 65536 ? 0 : 2 * A->cbw;       // 16-bit indices: the column, or the column within its block pair
  const bool want16 = mod16 <= 65536 && A->nnz > 0 && dz_opt(ctx, "spmv.col16", 1) != 0;
  if (A->col16 && (!want16 || A->col16_cap < A->nnz || changed_from == 0 || A->col16_mod != mod16)) {
    dz_big_put(ctx, A->col16);
    A->col16 = nullptr;
    A->col16_cap = 0;
  }
  if (want16 && (!A->col16 || changed_from >= 0)) {
    int64_t from = 0;
    if (!A->col16) {
      A->col16_cap = ((A->cap_nnz > A->nnz ? A->cap_nnz : A->nnz) + 3) & ~(int64_t)3;
      if (int rcp = dz_big_get(ctx, (size_t)A->col16_cap, &A->col16)) return rcp;
      A->col16_mod = mod16;
    } else {
      from = changed_from & ~(int64_t)3;
    }
    const int64_t cnt = A->nnz - from;
    if (cnt > 0)
      hipLaunchKernelGGL(k_narrow_cols, dim3(nblk((cnt + 3) / 4)), dim3(VB), 0, ctx->stream, cnt, A->col + from, A->col16 + from, mod16);
    DZ_HIP(hipGetLastError());
  }
  const int64_t np = A->m * (A->ncb + 1);
  if (np > 0) {   // a matrix without rows (an empty ray batch) has no block pointers
    if (int rcp = dz_big_get(ctx, (size_t)np, &A->cbptr)) return rcp;
    hipLaunchKernelGGL(k_colblock_ptr, dim3((unsigned)((np + VB - 1) / VB)), dim3(VB), 0, ctx->stream, A->m, A->ncb, A->cbw,
                       A->rowptr, A->col, A->cbptr);
    DZ_HIP(hipGetLastError());
  }
  int rc;
  A->vmax = 0.0f;
  A->split_row = A->m;
  A->long_avg = A->m > 0 ? (double)A->nnz / (double)A->m : 0.0;
  if (A->m > 0 && A->nnz > 0) {   // where the short tail of the matrix begins (see dazim_csr::split_row)
    float *pm;
    if ((rc = dz_scratch(ctx, "csr.absmax", (size_t)APART + 4, &pm))) return rc;
    unsigned long long *d_last = reinterpret_cast<unsigned long long *>(pm + APART + 2), h_last = 0;
    DZ_HIP(hipMemsetAsync(d_last, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_last_long_row, dim3(nblk(A->m)), dim3(VB), 0, ctx->stream, A->m, A->rowptr, SPLIT_SHORT, d_last);
    DZ_HIP(hipMemcpyAsync(&h_last, d_last, 8, hipMemcpyDeviceToHost, ctx->stream));
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    if ((int64_t)h_last < A->m && (int64_t)h_last > 0) {
      int64_t at = 0;
      DZ_HIP(hipMemcpy(&at, A->rowptr + h_last, 8, hipMemcpyDeviceToHost));
      A->split_row = (int64_t)h_last;
      A->long_avg = (double)at / (double)h_last;
    }
  }
  if (A->nnz > 0 && (rc = absmax_to_host(ctx, A->val, A->nnz, &A->vmax))) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}
bool dz_use_scatter(dazim_ctx *ctx, const dazim_csr *A) {
  if (dz_opt(ctx, "spmv.scatter", 1) == 0) return false;
  return A->cbptr && A->nnz >= (1 << 22) && A->m >= (int64_t)ctx->num_cu * SCW;
}
int dz_launch_spmvT(dazim_ctx *ctx, const dazim_csr *A, const float *y, float ymax, float *out, const float *beta_p,
                    float beta_sign, double *sumsq, int *npart, const int *guard) {
  const double pm = (double)A->vmax * (double)ymax;
  ctx->ksec["spmvt.kind"] = (dz_use_scatter(ctx, A) && std::isfinite(pm)) ? 1 : 0;
  ctx->ksec["spmvt.idx_bytes"] = (A->col16 && dz_use_scatter(ctx, A) && std::isfinite(pm)) ? 2 : 4;
  ctx->ksec["spmvt.lanes"] = 0;   // (the scatter form records its 64 or 16 lanes per row segment below)
  ctx->ksec["spmv.ncb"] = A->ncb;
  ctx->ksec["spmv.cbw"] = A->cbw;
  // non-finite values (NaN / Inf in G or y) cannot be put on the fixed-point grid: the gather form propagates them like
  // the reference's plain loop would (vmax and ymax come from k_absmax, which returns NaN / Inf if the array holds one)
  if (!dz_use_scatter(ctx, A) || !std::isfinite(pm)) {
    if (!A->colptr) {
      int rc0 = dz_build_transpose(ctx, const_cast<dazim_csr *>(A));
      if (rc0) return rc0;
    }
    const int gn = dz_spmv_blocks(ctx, A->n, A->m);
    if (npart) *npart = gn;
    return launch_spmv(ctx, A->n, A->m, A->colptr, A->row, A->tval, y, out, beta_p, beta_sign, sumsq, gn, guard);
  }
  int nchunk = ctx->num_cu / A->ncb;
  if (nchunk < 1) nchunk = 1;
  int rc;
  long long *part;
  if ((rc = dz_scratch(ctx, "spmvt.part", (size_t)nchunk * A->n, &part))) return rc;
  const double scale = fixed_scale(pm, A->m);
  const size_t lds = (size_t)A->cbw * 8;
  const RowSplit rs = row_split(ctx, A, 400.0 * A->ncb);   // measured: 16 lanes win at 141 and 296 entries per segment, 64 at 553
  ctx->ksec["spmvt.split_row"] = (double)rs.nsplit;
  const dim3 sgrid(nchunk * A->ncb), sblock(64 * SCW);
  rc = dispatch_rows(A, rs.shortseg, [&](auto gl, auto ng, auto *colp) -> int {
    using IT = std::remove_pointer_t<decltype(colp)>;
    const auto kern = spmvT_scatter<decltype(gl)::value, decltype(ng)::value, IT>;
    ctx->ksec["spmvt.lanes"] = decltype(gl)::value;
    DZ_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, sgrid, sblock, lds, ctx->stream, rs.nsplit, A->m, nchunk, A->ncb, A->cbw, A->n, A->cbptr,
                       (const IT *)colp, A->val, y, scale, part, guard, (sizeof(IT) == 2 && A->col16_mod > 0) ? 1 : 0);
    return 0;
  });
  if (rc) return rc;
  const int nb = nblk(A->n, NPART);
  hipLaunchKernelGGL(k_scatter_combine, dim3(nb), dim3(VB), 0, ctx->stream, A->n, nchunk, part, 1.0 / scale, out, beta_p,
                     beta_sign, sumsq, guard);
  DZ_HIP(hipGetLastError());
  if (npart) *npart = nb;
  return 0;
}

int dz_launch_spmvA(dazim_ctx *ctx, const dazim_csr *A, const float *x, float *out, const float *beta_p, float beta_sign,
                    double *sumsq, int *npart, const int *guard) {
  ctx->ksec["spmv.kind"] = use_blocked(ctx, A) ? 2 : (use_ldsx(ctx, A->m, A->n) ? 1 : 0);
  // index bytes streamed per entry (the whole-x LDS kernel needs the column itself, the blocked one takes either form)
  ctx->ksec["spmv.idx_bytes"] = (A->col16 && (use_blocked(ctx, A) || (use_ldsx(ctx, A->m, A->n) && A->col16_mod == 0))) ? 2 : 4;
  ctx->ksec["spmv.lanes"] = 0;   // (the column-blocked form records its 64 or 16 lanes per row segment below)
  ctx->ksec["spmv.ncb"] = A->ncb;
  ctx->ksec["spmv.cbw"] = A->cbw;
  if (!use_blocked(ctx, A)) {
    const int gm = dz_spmv_blocks(ctx, A->m, A->n);
    if (npart) *npart = gm;
    return launch_spmv(ctx, A->m, A->n, A->rowptr, A->col, A->val, x, out, beta_p, beta_sign, sumsq, gm, guard,
                       A->col16_mod == 0 ? A->col16 : nullptr);
  }
  const int npair = (A->ncb + 1) / 2;
  int nset = ctx->num_cu / npair;
  if (nset < 1) nset = 1;
  int rc;
  float *part;
  if ((rc = dz_scratch(ctx, "spmv.part", (size_t)npair * A->m, &part))) return rc;
  const size_t lds = (size_t)A->cbw * 2 * 4;
  const RowSplit rs = row_split(ctx, A, 600.0 * npair);    // measured: 16 lanes win at 282 and 519 entries per segment
  ctx->ksec["spmv.split_row"] = (double)rs.nsplit;
  const dim3 bgrid(nset * npair), bblock(64 * SCW);
  rc = dispatch_rows(A, rs.shortseg, [&](auto gl, auto ng, auto *colp) -> int {
    using IT = std::remove_pointer_t<decltype(colp)>;
    const auto kern = spmv_rows_blocked<decltype(gl)::value, decltype(ng)::value, IT>;
    ctx->ksec["spmv.lanes"] = decltype(gl)::value;
    DZ_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, bgrid, bblock, lds, ctx->stream, rs.nsplit, A->m, nset, npair, A->ncb, A->cbw, A->n, A->cbptr,
                       (const IT *)colp, A->val, x, part, guard, (sizeof(IT) == 2 && A->col16_mod > 0) ? 1 : 0);
    return 0;
  });
  if (rc) return rc;
  const int nb = nblk(A->m, NPART);
  hipLaunchKernelGGL(k_rows_combine, dim3(nb), dim3(VB), 0, ctx->stream, A->m, npair, part, out, beta_p, beta_sign, sumsq, guard);
  DZ_HIP(hipGetLastError());
  if (npart) *npart = nb;
  return 0;
}
int dz_scale_rows(dazim_ctx *ctx, dazim_csr *A, int64_t nrows, const float *w) {
  hipLaunchKernelGGL(k_scale_rows, dim3(dz_spmv_blocks(ctx, nrows, -1)), dim3(64 * WPB), 0, ctx->stream, nrows, A->rowptr, A->val, w);
  if (A->tperm) hipLaunchKernelGGL(k_gather_f, dim3(nblk(A->nnz)), dim3(VB), 0, ctx->stream, A->nnz, A->tperm, A->val, A->tval);
  DZ_HIP(hipGetLastError());
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return dz_build_colblocks(ctx, A, -1);
}

extern "C" {

int dz_csr_set_twin(dazim_ctx *ctx, dazim_csr *A, dazim_csr *B) {
  if (!A || !B || A->twin) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dz_csr_set_twin");
  A->twin = B;
  return 0;
}
// hand out the dense twin of a matrix built with option rays.dense_twin = 1 (NULL if there is none); the caller frees it
int dazim_csr_take_twin(dazim_ctx *ctx, dazim_csr *A, dazim_csr **twin) {
  if (!A || !twin) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_csr_take_twin");
  *twin = A->twin;
  A->twin = nullptr;
  return 0;
}

int dazim_csr_free(dazim_ctx *ctx, dazim_csr *A) {
  if (!A) return 0;
  if (A->twin) { dazim_csr *t = A->twin; A->twin = nullptr; (void)dazim_csr_free(ctx, t); }
  if (ctx) DZ_HIP(hipStreamSynchronize(ctx->stream));   // (a matrix may outlive its context: the arrays are still freed)
  else (void)hipDeviceSynchronize();
  void *ps[] = {A->rowptr, A->colptr, A->col, A->row, A->val, A->tval, A->tperm, A->cbptr, A->col16};
  for (void *p : ps)
    if (p) dz_big_put(ctx, p);
  delete A;
  return 0;
}

int dazim_csr_dims(const dazim_csr *A, int64_t *m, int64_t *n, int64_t *nnz) {
  if (!A) return DAZIM_E_BAD_ARG;
  if (m) *m = A->m;
  if (n) *n = A->n;
  if (nnz) *nnz = A->nnz;
  return 0;
}

int dazim_csr_from_coo(dazim_ctx *ctx, int64_t m, int64_t n, int64_t nnz, const int *irow_u,
                       const int *icol_u, const float *rw_u, dazim_csr **out) {
  if (!ctx || !out || m < 1 || n < 1 || nnz < 0 || nnz > 0xfffffff0ll || m > 0x7ffffff0 || n > 0x7ffffff0)
    return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_csr_from_coo");
  DZ_HIP(hipSetDevice(ctx->device));
  DzBuf<int> irow, icol;
  DzBuf<float> rw;
  int rc;
  if ((rc = irow.init(ctx, irow_u, nnz, true, false))) return rc;
  if ((rc = icol.init(ctx, icol_u, nnz, true, false))) return rc;
  if ((rc = rw.init(ctx, rw_u, nnz, true, false))) return rc;
  dazim_csr *A = new dazim_csr;
  auto fail = [&](int r) { dazim_csr_free(ctx, A); return r; };   // no leak on the error paths below
  A->m = m;
  A->n = n;
  A->nnz = nnz;
  const size_t nz = (size_t)(nnz > 0 ? nnz : 1);
  if ((rc = dz_big_get(ctx, (size_t)m + 1, &A->rowptr)) || (rc = dz_big_get(ctx, nz, &A->col)) || (rc = dz_big_get(ctx, nz, &A->val)))
    return fail(rc);
  unsigned *k0, *k1, *v0, *perm;
  int *bad;
  if ((rc = dz_scratch(ctx, "csr.k0", nz, &k0)) || (rc = dz_scratch(ctx, "csr.k1", nz, &k1)) ||
      (rc = dz_scratch(ctx, "csr.v0", nz, &v0)) || (rc = dz_scratch(ctx, "csr.perm", nz, &perm)) ||
      (rc = dz_scratch(ctx, "csr.bad", 4, &bad)))
    return fail(rc);
  DZ_HIP(hipMemsetAsync(bad, 0, 4, ctx->stream));
  const int nb = nblk(nnz);
  if (nnz > 0) {
    hipLaunchKernelGGL(k_check_range, dim3(nb), dim3(VB), 0, ctx->stream, nnz, irow.dev, 1, (int)m, bad);
    hipLaunchKernelGGL(k_check_range, dim3(nb), dim3(VB), 0, ctx->stream, nnz, icol.dev, 1, (int)n, bad);
    int hbad = 0;
    DZ_HIP(hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    if (hbad) {
      dazim_csr_free(ctx, A);
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "COO index outside 1..m / 1..n");
    }
    int rbits = 1, cbits = 1;
    while (((int64_t)1 << rbits) < m) rbits++;
    while (((int64_t)1 << cbits) < n) cbits++;
    // ---- canonical CSR: stable sort by column, then stable sort by row -> rows ascending, columns
    // ascending inside a row (entries of equal (row,col) keep the caller's order) ----
    unsigned *permc;
    if ((rc = dz_scratch(ctx, "csr.permc", nz, &permc))) return fail(rc);
    hipLaunchKernelGGL(k_iota_keys, dim3(nb), dim3(VB), 0, ctx->stream, nnz, icol.dev, k0, v0);
    size_t tb = 0, tb1 = 0;
    DZ_HIP(rocprim::radix_sort_pairs(nullptr, tb, k0, k1, v0, permc, (size_t)nnz, 0, cbits, ctx->stream));
    DZ_HIP(rocprim::radix_sort_pairs(nullptr, tb1, k0, k1, permc, perm, (size_t)nnz, 0, rbits, ctx->stream));
    if (tb1 > tb) tb = tb1;
    void *tmp;
    if ((rc = dz_scratch(ctx, "csr.tmp", tb + 256, &tmp))) return fail(rc);
    DZ_HIP(rocprim::radix_sort_pairs(tmp, tb, k0, k1, v0, permc, (size_t)nnz, 0, cbits, ctx->stream));
    hipLaunchKernelGGL(k_gather_i, dim3(nb), dim3(VB), 0, ctx->stream, nnz, permc, irow.dev, (int *)k0, -1);
    DZ_HIP(rocprim::radix_sort_pairs(tmp, tb, k0, k1, permc, perm, (size_t)nnz, 0, rbits, ctx->stream));
    hipLaunchKernelGGL(k_lower_bound, dim3(nblk(m + 1)), dim3(VB), 0, ctx->stream, m, nnz, k1, A->rowptr);
    hipLaunchKernelGGL(k_gather_f, dim3(nb), dim3(VB), 0, ctx->stream, nnz, perm, rw.dev, A->val);
    hipLaunchKernelGGL(k_gather_i, dim3(nb), dim3(VB), 0, ctx->stream, nnz, perm, icol.dev, A->col, -1);
    DZ_HIP(hipGetLastError());
  } else {
    DZ_HIP(hipMemsetAsync(A->rowptr, 0, (m + 1) * 8, ctx->stream));
  }
  if ((rc = dz_build_colblocks(ctx, A))) return fail(rc);
  if ((rc = dz_invalidate_transpose(A))) return fail(rc);
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  *out = A;
  return 0;
}

// take ownership of device CSR arrays (hipMalloc'ed: rowptr[m+1], col[nnz] 0-based, val[nnz])
int dazim_csr_adopt(dazim_ctx *ctx, int64_t m, int64_t n, int64_t nnz, int64_t *rowptr, int *col, float *val,
                    dazim_csr **out) {
  return dz_csr_adopt_cap(ctx, m, n, nnz, rowptr, col, val, 0, 0, out);
}

// (library-internal) the same for arrays that are larger than m / nnz (room for rows appended later, dazim_csr::cap_m): the
// capacities are known BEFORE the column blocks are built, so the 16-bit column copy is sized for the reserved entries once
// and an append only narrows its own tail
int dz_csr_adopt_cap(dazim_ctx *ctx, int64_t m, int64_t n, int64_t nnz, int64_t *rowptr, int *col, float *val,
                     int64_t cap_m, int64_t cap_nnz, dazim_csr **out) {
  if (!ctx || !out || !rowptr) return DAZIM_E_BAD_ARG;
  dazim_csr *A = new dazim_csr;
  A->m = m; A->n = n; A->nnz = nnz;
  A->rowptr = rowptr; A->col = col; A->val = val;
  if (cap_m > m) A->cap_m = cap_m;
  if (cap_nnz > nnz) A->cap_nnz = cap_nnz;
  int rc;
  if ((rc = dz_build_colblocks(ctx, A)) || (rc = dz_invalidate_transpose(A))) {
    dazim_csr_free(ctx, A);   // ownership was taken: the arrays go with it
    return rc;
  }
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  *out = A;
  return 0;
}

// B = the entries of A with |value| > tol, same shape and order.  The reference keeps two copies of every ray row: the
// triplets rw/iw/col hold the entries with |row| > ftol (inv/CalSurfG.f90:1358), the dense GVs/GGc/GGs every entry of the cells
// with |fdm| >= ftol (:1369-1378), and its residual diagnostics multiply with the dense ones (inv/CalSigamNorm.f90:73).  A
// program that wants both builds the matrix once with option rays.keep_small and derives the solver's matrix here: two
// streaming passes instead of tracing the rays twice.  reserve_rows / reserve_nnz: room for rows appended to B later.
int dazim_csr_threshold(dazim_ctx *ctx, const dazim_csr *A, float tol, int64_t reserve_rows, int64_t reserve_nnz, dazim_csr **out) {
  if (!ctx || !A || !out || reserve_rows < 0 || reserve_nnz < 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_csr_threshold");
  DZ_HIP(hipSetDevice(ctx->device));
  const int64_t m = A->m;
  int rc;
  long *cnt;
  if ((rc = dz_scratch(ctx, "thr.cnt", (size_t)(m + 1), &cnt))) return rc;
  int64_t *rowptr = nullptr;
  float *val = nullptr;
  int *col = nullptr;
  struct Arrays {
    dazim_ctx *c; int64_t *&rp; float *&v; int *&cl; bool keep = false;
    ~Arrays() { if (!keep) { dz_big_put(c, rp); dz_big_put(c, v); dz_big_put(c, cl); } }
  } arrays{ctx, rowptr, val, col};
  if ((rc = dz_big_get(ctx, (size_t)(m + reserve_rows + 1), &rowptr))) return rc;
  const unsigned nb = (unsigned)((m + 1 + 3) / 4);
  hipLaunchKernelGGL((k_threshold_rows<false>), dim3(nb), dim3(256), 0, ctx->stream, m, A->rowptr, A->col, A->val, tol, cnt,
                     (const long *)nullptr, (int *)nullptr, (float *)nullptr);
  size_t tb = 0;
  DZ_HIP(rocprim::exclusive_scan(nullptr, tb, cnt, (long *)rowptr, 0l, (size_t)(m + 1), rocprim::plus<long>(), ctx->stream));
  void *p;
  if ((rc = dz_scratch(ctx, "thr.scan", tb + 256, &p))) return rc;
  DZ_HIP(rocprim::exclusive_scan(p, tb, cnt, (long *)rowptr, 0l, (size_t)(m + 1), rocprim::plus<long>(), ctx->stream));
  long nnz = 0;
  DZ_HIP(hipMemcpyAsync(&nnz, rowptr + m, 8, hipMemcpyDeviceToHost, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t cap = nnz + reserve_nnz;
  if ((rc = dz_big_get(ctx, (size_t)(cap > 0 ? cap : 1), &val)) || (rc = dz_big_get(ctx, (size_t)(cap > 0 ? cap : 1), &col))) return rc;
  hipLaunchKernelGGL((k_threshold_rows<true>), dim3(nb), dim3(256), 0, ctx->stream, m, A->rowptr, A->col, A->val, tol, cnt,
                     (const long *)rowptr, col, val);
  DZ_HIP(hipGetLastError());
  arrays.keep = true;
  return dz_csr_adopt_cap(ctx, m, A->n, nnz, rowptr, col, val, m + reserve_rows, cap, out);
}

// append rows m+1..m+extra_m given as COO (1-based absolute row ids, any order) -- the reference
// appends its Tikhonov rows to the same rw/iw/col arrays (inv/TikhRegul.f90:2)
int dazim_csr_append_coo(dazim_ctx *ctx, dazim_csr *A, int64_t extra_m, int64_t nnz2, const int *irow_u,
                         const int *icol_u, const float *rw_u) {
  if (!ctx || !A || extra_m < 0 || nnz2 < 0) return DAZIM_E_BAD_ARG;
  if (extra_m == 0 && nnz2 == 0) return 0;
  // build the block as its own matrix with rows shifted to 1..extra_m
  DzBuf<int> irow;
  int rc;
  if ((rc = irow.init(ctx, irow_u, nnz2, true, false))) return rc;
  int *shifted;
  if ((rc = dz_scratch(ctx, "csr.shift", (size_t)(nnz2 > 0 ? nnz2 : 1), &shifted))) return rc;
  if (nnz2 > 0) hipLaunchKernelGGL(k_gather_i, dim3(nblk(nnz2)), dim3(VB), 0, ctx->stream, nnz2, (const unsigned *)nullptr, irow.dev, shifted, (int)-A->m);
  dazim_csr *B = nullptr;
  if ((rc = dazim_csr_from_coo(ctx, extra_m > 0 ? extra_m : 1, A->n, nnz2, shifted, icol_u, rw_u, &B))) return rc;
  const int64_t m2 = A->m + extra_m, nz2 = A->nnz + nnz2;
  if (A->cap_m >= m2 && A->cap_nnz >= nz2) {   // the arrays were allocated with room for these rows: append in place
    const int64_t nnz1 = A->nnz;
    if (extra_m > 0)
      hipLaunchKernelGGL(k_offset_ptr, dim3(nblk(extra_m + 1)), dim3(VB), 0, ctx->stream, extra_m + 1, B->rowptr, A->nnz, A->rowptr + A->m);
    DZ_HIP(hipMemcpyAsync(A->col + nnz1, B->col, (size_t)nnz2 * 4, hipMemcpyDeviceToDevice, ctx->stream));
    DZ_HIP(hipMemcpyAsync(A->val + nnz1, B->val, (size_t)nnz2 * 4, hipMemcpyDeviceToDevice, ctx->stream));
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    dazim_csr_free(ctx, B);
    A->m = m2;
    A->nnz = nz2;
    if ((rc = dz_build_colblocks(ctx, A, nnz1 > 0 ? nnz1 : 0))) return rc;
    if ((rc = dz_invalidate_transpose(A))) return rc;
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
  }
  int64_t *rowptr;
  int *col;
  float *val;
  if ((rc = dz_big_get(ctx, (size_t)(m2 + 1), &rowptr)) || (rc = dz_big_get(ctx, (size_t)(nz2 > 0 ? nz2 : 1), &col)) ||
      (rc = dz_big_get(ctx, (size_t)(nz2 > 0 ? nz2 : 1), &val)))
    return rc;
  DZ_HIP(hipMemcpyAsync(rowptr, A->rowptr, (A->m + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
  if (extra_m > 0)
    hipLaunchKernelGGL(k_offset_ptr, dim3(nblk(extra_m + 1)), dim3(VB), 0, ctx->stream, extra_m + 1, B->rowptr, A->nnz, rowptr + A->m);
  DZ_HIP(hipMemcpyAsync(col, A->col, (size_t)A->nnz * 4, hipMemcpyDeviceToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync(val, A->val, (size_t)A->nnz * 4, hipMemcpyDeviceToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync(col + A->nnz, B->col, (size_t)nnz2 * 4, hipMemcpyDeviceToDevice, ctx->stream));
  DZ_HIP(hipMemcpyAsync(val + A->nnz, B->val, (size_t)nnz2 * 4, hipMemcpyDeviceToDevice, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  dazim_csr_free(ctx, B);
  dz_big_put(ctx, A->rowptr);
  dz_big_put(ctx, A->col);
  dz_big_put(ctx, A->val);
  A->rowptr = rowptr; A->col = col; A->val = val;
  A->m = m2; A->nnz = nz2;
  A->cap_m = A->cap_nnz = 0;
  if ((rc = dz_build_colblocks(ctx, A))) return rc;
  if ((rc = dz_invalidate_transpose(A))) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// copy the matrix out as the reference's COO triplets (1-based), rows ascending
int dazim_csr_to_coo(dazim_ctx *ctx, const dazim_csr *A, int *irow_u, int *icol_u, float *rw_u) {
  if (!ctx || !A) return DAZIM_E_BAD_ARG;
  DzBuf<int> irow, icol;
  DzBuf<float> rw;
  int rc;
  if ((rc = irow.init(ctx, irow_u, A->nnz, false, true))) return rc;
  if ((rc = icol.init(ctx, icol_u, A->nnz, false, true))) return rc;
  if ((rc = rw.init(ctx, rw_u, A->nnz, false, true))) return rc;
  if (A->nnz > 0) {
    unsigned *rowid;
    if ((rc = dz_scratch(ctx, "csr.perm", (size_t)A->nnz, &rowid))) return rc;
    hipLaunchKernelGGL(k_expand_rows, dim3(dz_spmv_blocks(ctx, A->m, -1)), dim3(64 * WPB), 0, ctx->stream, A->m, A->rowptr, rowid);
    const int nb = nblk(A->nnz);
    if (irow.dev) hipLaunchKernelGGL(k_gather_i, dim3(nb), dim3(VB), 0, ctx->stream, A->nnz, (const unsigned *)nullptr, (const int *)rowid, irow.dev, 1);
    if (icol.dev) hipLaunchKernelGGL(k_gather_i, dim3(nb), dim3(VB), 0, ctx->stream, A->nnz, (const unsigned *)nullptr, A->col, icol.dev, 1);
    if (rw.dev) DZ_HIP(hipMemcpyAsync(rw.dev, A->val, (size_t)A->nnz * 4, hipMemcpyDeviceToDevice, ctx->stream));
    DZ_HIP(hipGetLastError());
  }
  if ((rc = irow.finish()) || (rc = icol.finish()) || (rc = rw.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int dazim_csr_scale_rows(dazim_ctx *ctx, dazim_csr *A, const float *w_u) {
  if (!ctx || !A || !w_u) return DAZIM_E_BAD_ARG;
  DzBuf<float> w;
  int rc;
  if ((rc = w.init(ctx, w_u, A->m, true, false))) return rc;
  return dz_scale_rows(ctx, A, A->m, w.dev);
}

int dazim_csr_col_abs_sums(dazim_ctx *ctx, const dazim_csr *A, float *out_u) {
  if (!ctx || !A || !out_u) return DAZIM_E_BAD_ARG;
  DzBuf<float> out;
  int rc;
  if ((rc = out.init(ctx, out_u, A->n, false, true))) return rc;
  unsigned long long *acc;
  if ((rc = dz_scratch(ctx, "csr.colacc", (size_t)A->n, &acc))) return rc;
  DZ_HIP(hipMemsetAsync(acc, 0, (size_t)A->n * 8, ctx->stream));
  const double scale = fixed_scale((double)A->vmax, A->m);
  if (A->nnz) hipLaunchKernelGGL(k_col_abs_sums, dim3(nblk(A->nnz)), dim3(VB), 0, ctx->stream, A->nnz, A->col, A->val, scale, acc);
  hipLaunchKernelGGL(k_fixed_to_float, dim3(nblk(A->n)), dim3(VB), 0, ctx->stream, A->n, acc, 1.0 / scale, out.dev);
  DZ_HIP(hipGetLastError());
  if ((rc = out.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// aprod, inv/aprod.f90:7
int dazim_aprod(dazim_ctx *ctx, int mode, const dazim_csr *A, float *x_u, float *y_u) {
  if (!ctx || !A || !x_u || !y_u || (mode != 1 && mode != 2)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_aprod");
  DZ_HIP(hipSetDevice(ctx->device));
  DzBuf<float> x, y;
  int rc;
  if ((rc = x.init(ctx, x_u, A->n, true, mode == 2))) return rc;
  if ((rc = y.init(ctx, y_u, A->m, true, mode == 1))) return rc;
  if (mode == 1) {
    DzTimer t(ctx, "spmv");
    if ((rc = dz_launch_spmvA(ctx, A, x.dev, y.dev, nullptr, 1.0f, nullptr, nullptr))) return rc;
    t.stop();
  } else {
    float ymax = 1.0f;
    if (dz_use_scatter(ctx, A)) {   // fixed-point scale needs max|y| (inside LSMR it is 1: u is normalised)
      if ((rc = absmax_to_host(ctx, y.dev, A->m, &ymax))) return rc;
      DZ_HIP(hipStreamSynchronize(ctx->stream));
    }
    DzTimer t(ctx, "spmvt");
    if ((rc = dz_launch_spmvT(ctx, A, y.dev, ymax, x.dev, nullptr, 1.0f, nullptr, nullptr))) return rc;
    t.stop();
  }
  if ((rc = x.finish()) || (rc = y.finish())) return rc;
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
