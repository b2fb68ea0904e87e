// rays.hip -- K4 + K5 of SURVEY.md: receiver traveltimes (srtimes, inv/CalSurfG.f90:1599), ray
// back-tracing with B-spline Frechet weights (rpaths, :1735) and G-row assembly (:1339-1364) for a
// batch of rays whose eikonal fields are already resident in HBM (output of dazim_fmm_batch).
//
// Eight rays per wavefront, one per 8-lane group (the kernel is bound by instruction issue and by the dependent
// loads of a step, so SIMT across groups divides the instruction count per ray and multiplies the loads in flight;
// measured: 16 lanes per ray 0.094 s, 8 lanes 0.073 s, 4 lanes 0.084 s on the S-256 batch).  The half-cell stepping
// is inherently serial and is executed redundantly by the lanes of a group, while the 4x4 B-spline scatter of every
// sub-segment is spread over them: each lane keeps two cells of the current 4x4 block of the Frechet grid(s) in
// registers and the block is written back to the ray's grid in HBM scratch only when the ray leaves it.  Touched cells are collected in an
// LDS cell list.  The grid of a ray (its "slot") is stored in the order the list wants it (jj the row, kk contiguous) and is all zeros
// between rays: a ray remembers the range of B-spline blocks it has been in, looks for its cells in that range only and puts zeros
// back into it, so the work per ray follows the ray and not the grid.  Rows are emitted straight into CSR in the reference's column order (depth-major, then jj,
// kk) by a count pass, an exclusive scan and an emit pass that reuses the saved cell lists -- no atomics, so G
// is reproducible.  fp32 without FMA like the reference.
#include <cmath>
#include <chrono>
#include <unistd.h>

#include "dazim_internal.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

#ifdef DZ_RAYS_MARK   // experiment-only build: phase markers in the assembly (tools/rays_phase_count.py counts the instructions between them)
#define RAYS_MARK(i) asm volatile("; MARK " #i ::: "memory")
#else
#define RAYS_MARK(i)
#endif

constexpr int GDX = 5, GDZ = 5;
constexpr int RM = DAZIM_RMAX;
constexpr float EARTH = 6371.0f;
constexpr float FTOL = 1e-4f;  // inv/CalSurfG.f90:999

struct RayArgs {
  dazim_geom g;
  int nx, ny, nz, kmax;
  long nray;
  const int *field;     // [nray] field of each ray
  const float *rcx, *rcz;
  const float *scx, *scz;  // [nfield]
  const int *period;       // [nfield], 1-based (velocity map of the field)
  const int *kidx;         // [nfield], 1-based period slot of the depth kernels (knumi), may equal period
  const float *veln;       // [kmax][nnx][nnz]
  const float *ttn;        // [nfield][nnx][nnz]; TILED kernels: the fields as dazim_fmm_batch(ttn = NULL) left them, node (x0, z0) of field f
                           // at ttn[(tslot ? tslot[f] : f) * fstride + dz_tile_x(x0, tsh) + dz_tile_z(z0)] (4 x 4 tiles: a ray that
                           // moves in x stays in one 64-byte tile for four nodes instead of touching a new 128-byte line per node)
  const int *tslot;
  int tsh;
  long fstride;
  // beside an asynchronous eikonal launch (option fmm.async): defer_mark[quad] != 0 = not traced yet; a pass traces the marked quads
  // whose fields are finished (fdone[f] = 1; 0 still marching, 2 band overflow: the host reruns the field first) and unmarks them
  const int *fdone;
  int *defer_mark;
  int max_quads;           // > 0: a workgroup leaves after tracing that many quads
  int sweeps;              // > 1: the pass offers every quad of a range that many times (see the queue of rays_kernel)
  const float *ttnr;       // [nfield][RM][RM]
  const int *nstsr;        // [nfield][RM][RM]
  const dazim_refbox *boxes;
  const float *vels;       // [nz][ny][nx]
  const double *svs, *svp, *srho;  // [nz][kmax][nx*ny]
  unsigned nvx_magic;      // ceil(2^32 / nvx): cell id / nvx = __umulhi(id, nvx_magic) for every id < 65 536 (checked on the host)
  const double *skern;     // [nz][kmax][nx*ny] svp*coe_a + srho*coe_rho + svs per model cell and period (k_row_kernels), or nullptr
  const float *lsen;       // joint mode: Lsen_Gsc [nz-1][kmax][nx*ny] (fp32, inv/CalSurfGAniso_Joint.f90:337)
  // double-precision reciprocals RN(1/d) of the loop-invariant fp32 divisors (grid spacings and 2*EARTH*spacing): see divr()
  double r_dnx, r_dnz, r_dnxr, r_dnzr, r_dvx, r_dvz, r_e2dnx, r_e2dnxr;
  float dplh;              // min cell size (before the 0.5 factor), host libm
  float *dsurf;            // [nray]
  int *status;             // [nray]
  int *rbflag;             // [nray]
  long *count;             // [nray]  (count pass out)
  int *nlist;              // [nray]  cells with |fdm| >= ftol saved by the count pass (-1: did not fit, retrace)
  unsigned short *lcell;   // [nray][LK] their (jj,kk) cell ids, ascending
  float *lval;             // [nray][LK] (x3 in joint mode) their fdm (, fdmc, fdms) values
  float *fdm_scratch;      // [nwg*8][nvz+2][nvx+2] (x3 in joint mode): one Frechet grid slot per lane group, all zeros between rays
  int LK;
  int lcap;                // LDS cell-list capacity per ray
  const unsigned *perm;    // [nray] order in which the rays are dealt to the lane groups: by field, then by source-receiver
                           // distance, so that the rays marching in lockstep in one wavefront have similar lengths (speed only:
                           // everything a ray produces is stored under its own index)
  unsigned *qcount;        // [16] task counters of the two passes (8 ranges each, one per XCD); [16] rays whose cell list outgrew
                           // the LDS capacity (full-grid sweep), [17] rays whose list outgrew LK (traced again by the emit pass);
                           // [18] quads a pass beside an asynchronous eikonal launch left for a later pass
  float2 *pts;             // option rays.keep_paths: [nray][pcap] ray-path points (colatitude, longitude in rad) as the reference's
  int *npts;               //   rgx/rgz(1:nrp) (receiver first, source last; fwd/rpathsAzim.f90:221-380); npts = nrp, or -1 if > pcap
  int pcap;
  int dense;               // the reference's dense copies GVs/GGc/GGs as a second matrix ("twin", option rays.dense_twin):
                           // 0 off; 2 (count pass): also count the twin's entries into countd; 1 (a second emit pass): write the
                           // twin -- every non-zero entry of the |fdm| >= ftol cells, the dVs block with the Brocher derivatives
                           // coe_a / coe_rho of the LAST such cell of the ray, which is what the reference's second loop uses
                           // (inv/CalSurfG.f90:1369-1378, inv/CalSurfGAniso_Joint.f90:759-775 do not recompute them)
  long *countd;            // [nray] twin entries per row (count pass out when dense = 2)
  int plain_step;          // option rays.plain_step (test knob): the stepping loop never carries a value over, always takes the general
                           // vel_at and always does the refined-box work -- a second route to the same bits
  int keep_small;          // 1: keep every non-zero row entry of the |fdm| >= ftol cells (the forward program's dense GGc/GGs,
                           // fwd/FwdTraveltimeCPS.f90:694-712); 0: the inversion's second |row| > ftol threshold
  const long *rowptr;      // [nray+1] (emit pass in)
  float *val;
  int *col;
};

// sin of a colatitude x in (0, pi): sin x = cos(x - pi/2), an even Taylor polynomial to y^18 in fp64
// (remainder < 3e-14 for |y| <= pi/2), rounded to fp32 -- the correctly rounded fp32 sine up to ties
// nobody will hit, at a tenth of the cost of the general fp64 sin.  Outside (0, pi) fall back to it.
__device__ __forceinline__ float dz_sinf(float x) {
  if (!(x > 0.0f && x < 3.1415927f)) return (float)sin((double)x);
  const double y = (double)x - 1.5707963267948966192;
  const double y2 = y * y;
  double p = -1.5619206968586226e-16;            // -1/18!
  p = fma(p, y2, 4.7794773323873853e-14);        //  1/16!
  p = fma(p, y2, -1.1470745597729725e-11);       // -1/14!
  p = fma(p, y2, 2.0876756987868099e-09);        //  1/12!
  p = fma(p, y2, -2.7557319223985891e-07);       // -1/10!
  p = fma(p, y2, 2.4801587301587302e-05);        //  1/8!
  p = fma(p, y2, -1.3888888888888889e-03);       // -1/6!
  p = fma(p, y2, 4.1666666666666664e-02);        //  1/4!
  p = fma(p, y2, -0.5);
  p = fma(p, y2, 1.0);
  return (float)p;
}

// azimuth of the step (x0,z0) -> (x1,z1): azdist (inv/rpathsAzim.f90:687-793) with the reference's
// implicit typing, called as at inv/rpathsAzim.f90:415-423; returns cos(2 psi), sin(2 psi)
__device__ __forceinline__ void step_azimuth(float x0, float z0, float x1, float z1, float &c2psi, float &s2psi) {
  const float PI_F = 3.1415926535898f;
  const float evtlat = (PI_F / 2 - x0) * 180.0f / PI_F, evtlon = z0 * 180.0f / PI_F;
  const float stalat = (PI_F / 2 - x1) * 180.0f / PI_F, stalon = z1 * 180.0f / PI_F;
  const double pi = (double)3.1415926535898f;
  const float piby2 = (float)(pi / (double)2.f);
  const double rad = (double)2.f * pi / (double)360.f;
  const double sph = (double)(1.0f / 298.257f);
  const double scolat = (double)piby2 - atan((1. - sph) * (1. - sph) * tan((double)stalat * rad));
  const double ecolat = (double)piby2 - atan((1. - sph) * (1. - sph) * tan((double)evtlat * rad));
  const double slon = (double)stalon * rad, elon = (double)evtlon * rad;
  const double a = sin(scolat) * cos(slon), b = sin(scolat) * sin(slon), c = cos(scolat);
  const double dd = sin(elon), ee = -cos(elon), cc = cos(ecolat);
  const double gg = -cc * ee, hh = cc * dd, kk = -sin(ecolat);
  const double rhs1 = (a - dd) * (a - dd) + (b - ee) * (b - ee) + c * c - (double)2.f;
  const double rhs2 = (a - gg) * (a - gg) + (b - hh) * (b - hh) + (c - kk) * (c - kk) - (double)2.f;
  double daz = atan2(rhs1, rhs2);
  if (daz < 0.0) daz = daz + 2 * pi;
  float az = (float)(daz / rad);
  if (fabsf(az - 360.f) < .00001f) az = 0.0f;
  const float rgpsi = az / 180 * PI_F;
  c2psi = (float)cos((double)(2.0f * rgpsi));
  s2psi = (float)sin((double)(2.0f * rgpsi));
}

// x / d, correctly rounded, for a divisor whose double-precision reciprocal rd = RN(1/d) is at hand: three instructions
// (convert, multiply, convert) instead of the ~11 of the IEEE fp32 division sequence -- a fifth to a third of this kernel was
// divisions by grid spacings.  Exact for EVERY x: the double product is within 2^-52 (relative) of x/d, and the quotient of two
// 24-bit numbers X/D is either a 24-bit number itself or at least 1/(D*M) >= 2^-49 (relative) away from every rounding
// boundary M of the 24-bit format (|X*2^k - D*M| is a non-zero integer; a quotient cannot sit exactly on a boundary, because
// X = D'*M with an odd 25-bit M would need more than 24 bits), so rounding the double to fp32 rounds where the exact quotient
// rounds.  Infinities, NaNs and zeros come out as the division's.
__device__ __forceinline__ float divr(float x, double rd) { return (float)((double)x * rd); }

__device__ __forceinline__ void basis(float v, float b[4]) {  // inv/CalSurfG.f90:2145-2148
  const float om = 1.0f - v;
  b[0] = om * om * om / 6.0f;
  b[1] = (4.0f - 6.0f * (v * v) + 3.0f * (v * v * v)) / 6.0f;
  b[2] = (1.0f + 3.0f * v + 3.0f * (v * v) - 3.0f * (v * v * v)) / 6.0f;
  b[3] = v * v * v / 6.0f;
}

// x / 6.0f through divr (the reciprocal is a compile-time constant)
__device__ __forceinline__ float div6(float x) { return divr(x, 1.0 / 6.0); }
// element i (0..3) of the cubic B-spline basis at v, inv/CalSurfG.f90:2145-2148: only the selected numerator is formed and divided
// (the kernel is bound by instruction issue; the four divisions of the plain form were a fifth of a step).  i is a constant of the lane at every call site (hoisted, or folded where the compiler knows
// its range).  Elements 0 and 3 are the cube of w = 1 - v or v; elements 1 and 2 are (p + c * w^2) + d * w^3 with w = v and
// (p, c, d) = (4, -6, 3) or (1 + 3 v, 3, -3): the reference's sums in the reference's order, x + (-k) * y for its x - k * y (the
// same number: negation is exact).  tools/check_basis.c compares this with the plain four-numerator form over all fp32 patterns.
__device__ __forceinline__ float basis1(float v, int i) {
  const float w = i == 0 ? 1.0f - v : v;
  const float t2 = w * w, t3 = t2 * w;
  const float p = i == 1 ? 4.0f : 1.0f + 3.0f * v;
  const float c = i == 1 ? -6.0f : 3.0f, d = i == 1 ? 3.0f : -3.0f;
  const float n = (p + c * t2) + d * t3;
  return div6((i == 0 || i == 3) ? t3 : n);
}

// bilinear velocity inside coarse cell (ipx,ipz), inv/CalSurfG.f90:2129-2137
__device__ __forceinline__ float vel_at(const dazim_geom &g, const float *veln, int ipx, int ipz, float drx, float drz,
                                        double rdnx, double rdnz) {
  float vel = 0.0f;
#pragma unroll
  for (int l = 1; l <= 2; l++)
#pragma unroll
    for (int m = 1; m <= 2; m++) {
      float produ = (1.0f - fabsf(divr((float)(m - 1) * g.dnz - drz, rdnz)));
      produ = produ * (1.0f - fabsf(divr((float)(l - 1) * g.dnx - drx, rdnx)));
      if (ipz - 1 + m <= g.nnz && ipx - 1 + l <= g.nnx && ipz - 1 + m >= 1 && ipx - 1 + l >= 1)
        vel = vel + veln[(size_t)(ipx - 2 + l) * g.nnz + (ipz - 2 + m)] * produ;
    }
  return vel;
}
// the same for a cell that touches neither the last row nor the last column of the grid (1 <= ipx < nnx, 1 <= ipz < nnz): all four
// bounds tests of vel_at pass there, so the four terms are added unconditionally, in the same order
__device__ __forceinline__ float vel_at_interior(const dazim_geom &g, const float *veln, int ipx, int ipz, float drx, float drz,
                                                 double rdnx, double rdnz) {
  float vel = 0.0f;
#pragma unroll
  for (int l = 1; l <= 2; l++)
#pragma unroll
    for (int m = 1; m <= 2; m++) {
      float produ = (1.0f - fabsf(divr((float)(m - 1) * g.dnz - drz, rdnz)));
      produ = produ * (1.0f - fabsf(divr((float)(l - 1) * g.dnx - drx, rdnx)));
      vel = vel + veln[(size_t)(ipx - 2 + l) * g.nnz + (ipz - 2 + m)] * produ;
    }
  return vel;
}

// bilinear(nv,dsx,dsz), inv/CalSurfG.f90:2293 -- velocity at a point of cell (cx,cz)
__device__ __forceinline__ float bilin_cell(const dazim_geom &g, const float *veln, int cx, int cz, float px, float pz,
                                            double rdnx, double rdnz) {
  const float drx = (px - g.gox) - (float)(cx - 1) * g.dnx;
  const float drz = (pz - g.goz) - (float)(cz - 1) * g.dnz;
  float biv = 0.0f;
#pragma unroll
  for (int i = 1; i <= 2; i++)
#pragma unroll
    for (int j = 1; j <= 2; j++) {
      const float produ = (1.0f - fabsf(divr((float)(i - 1) * g.dnx - drx, rdnx))) *
                          (1.0f - fabsf(divr((float)(j - 1) * g.dnz - drz, rdnz)));
      biv = biv + veln[(size_t)(cx - 2 + i) * g.nnz + (cz - 2 + j)] * produ;
    }
  return biv;
}

// The factor of a dVs row entry that does not depend on the ray (inv/CalSurfG.f90:1339-1364): the Brocher derivatives of the cell's
// velocity and the three depth kernels, (svp*coe_a + srho*coe_rho + svs) in the reference's order and precision (dz_row_kernel,
// dazim_internal.h, which dazim_vs_kernels shares) -- once per model cell, layer and period instead of once per ray that crosses the cell (both passes of rays_kernel; the emit pass is little else).
__global__ void k_row_kernels(long n, int kmax, long ncol, const float *__restrict__ vels, const double *__restrict__ svs,
                              const double *__restrict__ svp, const double *__restrict__ srho, double *__restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // (layer, period, column)
  if (i >= n) return;
  const long k = i / (kmax * ncol), c = i % ncol;
  out[i] = dz_row_kernel(vels[k * ncol + c], svs[i], svp[i], srho[i]);
}

// sort key of a ray for the order in which rays are dealt to the wavefronts: field in the high bits, quantised source-receiver
// distance (a proxy for the number of steps of the ray) in the low `dbits`
__global__ void k_ray_keys(long nray, const int *__restrict__ field, const float *__restrict__ scx, const float *__restrict__ scz,
                           const float *__restrict__ rcx, const float *__restrict__ rcz, float inv_dmax, int dbits,
                           unsigned *__restrict__ keys, unsigned *__restrict__ iota, const int *__restrict__ order) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nray) return;
  const int f = field[i];
  const float dx = scx[f] - rcx[i], dz = (scz[f] - rcz[i]) * __sinf(rcx[i]);
  const float d = sqrtf(dx * dx + dz * dz) * inv_dmax;
  const unsigned dmaxq = (1u << dbits) - 1u;
  unsigned q = d >= 1.0f ? dmaxq : (unsigned)(d * (float)dmaxq);
  // (order: the fields' places in the eikonal launch's queue -- beside an asynchronous launch the rays come in the order their fields finish)
  keys[i] = ((unsigned)(order ? order[f] : f) << dbits) | (dmaxq - q);          // longest rays of a field first
  iota[i] = (unsigned)i;
}

// lanes per ray: 8 in the count pass, which traces every ray (measured: 16 lanes 94 ms, 8 lanes 73 ms, 4 lanes 84 ms on the S-256
// batch); 16 in the emit pass, which only walks the saved cell lists (lane-parallel work: 8.2 ms with 16 lanes, 12.5 with 8)
constexpr int GP_COUNT = 8, GP_EMIT = 16;   // (count pass, whole step: 4 and 16 lanes per ray are both 17 % slower at S-256)
constexpr int RAYS_MINW = 4;   // wavefronts per SIMD the isotropic forms of rays_kernel are compiled for (the azimuthal ones: 2)
constexpr int RPW_MAX = 64 / GP_COUNT;   // rays per wavefront (most of the two passes: sizes the scratch slots)
__device__ __forceinline__ void cbar() { asm volatile("" ::: "memory"); }  // compiler-only barrier (same-wave ops are in order)

// One GP-lane group per ray (~330 k instructions per ray when one wavefront traced one ray, all of it per-ray
// scalar work except the 4x4 B-spline scatter).  The Frechet grid(s) of a ray live in an HBM scratch slot; the
// 4x4 block currently being updated is cached in registers, LPR cells per lane, and written back when the ray
// moves to another B-spline cell (every ~10 steps), so every cell still sees its contributions in the
// reference's order (fdm = r1 + fdm).
// MAP: the rows of the per-period map inversion (dazim_rays_build_G_maps) -- the Frechet values fdm (, fdmc, fdms) themselves,
// one column block per period: what the 3-D rows are with unit depth kernels and nz = 2, the period folded into the column.
template <bool EMIT, bool AZIM, bool TILED, bool MAP>
__global__ __launch_bounds__(64, AZIM ? 2 : RAYS_MINW) void rays_kernel(RayArgs A_) {
  // (arguments through an opaque pointer to the kernarg segment, like fmm_kernel: taken by value, the ~50 scalar registers of
  // RayArgs stay alive across the stepping loop and the spill code moved 93 of its 1 227 VALU instructions per step through
  // VGPR lanes -- v_readlane / v_writelane --, 17 more through scratch memory)
  using ArgP = const __attribute__((address_space(4))) RayArgs *;
  auto launder = [](ArgP p) {
    int z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return (ArgP)((const __attribute__((address_space(4))) char *)p + __builtin_amdgcn_readfirstlane(z));
  };
  ArgP Ap = launder((ArgP)__builtin_amdgcn_kernarg_segment_ptr());
#define A (*Ap)
#define RAYS_ARGS_FRESH Ap = launder(Ap)
  constexpr int GP = EMIT ? GP_EMIT : GP_COUNT;   // lanes per ray
  constexpr int RPW = 64 / GP;                    // rays per wavefront
  constexpr int LPR = 16 / GP;                    // cells of the 4x4 B-spline block per lane
  constexpr int LSTEP = 4 / LPR;                  // ... which are LSTEP rows apart
  constexpr unsigned GMASK = (1u << GP) - 1u;
  extern __shared__ __attribute__((aligned(16))) unsigned short s_lists[];  // [RPW][lcap] cell lists
  dazim_geom g;
  g.nvx = A.g.nvx; g.nvz = A.g.nvz; g.nnx = A.g.nnx; g.nnz = A.g.nnz;
  g.gox = A.g.gox; g.goz = A.g.goz; g.dnx = A.g.dnx; g.dnz = A.g.dnz; g.dvx = A.g.dvx; g.dvz = A.g.dvz;
  const int lane = threadIdx.x, grp = lane / GP, gl = lane & (GP - 1);
  const int lm = gl & 3, l0 = gl >> 2;  // this lane's cells of the 4x4 scatter: (m, l) = (lm, l0 + q*LSTEP), q < LPR
  const int nnx = g.nnx, nnz = g.nnz, nvx = g.nvx, nvz = g.nvz;
  const int ldf = nvx + 2, nf = ldf * (nvz + 2);   // the slot: cell (jj, kk) at jj * ldf + kk, 0 <= jj <= nvz + 1, 0 <= kk <= nvx + 1
  constexpr int NG = AZIM ? 3 : 1;
  const unsigned nvx_magic = A.nvx_magic;   // (cell ids are decoded in the innermost loops of the row assembly: two instructions instead of the ~20 of an integer division)
  const int LC = A.lcap;   // list capacity (<= 1024 so that 12 wavefronts fit a CU); longer lists fall back to a full-grid sweep
  unsigned short *s_list = s_lists + (size_t)grp * LC;
  float *gfdm = A.fdm_scratch + ((size_t)blockIdx.x * RPW + grp) * nf * NG;
  float *gfdmc = gfdm + nf, *gfdms = gfdm + 2 * nf;
  // The slot is ALL ZEROS whenever its group takes a ray (the host clears the scratch once per call; every ray clears what it wrote).
  // s_rng: the B-spline blocks (cbx, cbz) the ray being traced has been in -- min cbx, min cbz, max cbx, max cbz --, kept in LDS so
  // that the stepping loop holds no register for it; the ray's non-zero cells lie in kk = min cbx .. max cbx + 3, jj likewise.
  __shared__ int s_rngs[RPW][4];
  int *s_rng = s_rngs[grp];
  constexpr int RC = 8;   // cells per lane of the row assembly's register form (see `usual` below)
  const float gox = g.gox, goz = g.goz, dnx = g.dnx, dnz = g.dnz, dvx = g.dvx, dvz = g.dvz;
  const double rdnx = A.r_dnx, rdnz = A.r_dnz, rdnxr = A.r_dnxr, rdnzr = A.r_dnzr, rdvx = A.r_dvx, rdvz = A.r_dvz;
  const unsigned gmask_shift = grp * GP;
  // XCD-aware order (speed only): workgroup b runs on XCD b % 8, and the rays of one field read the
  // same traveltime grids, so each XCD gets one contiguous eighth of the ray quads.  Within its eighth a workgroup takes
  // the next quad from a counter (rays differ in length by an order of magnitude: equal shares of quads are not equal
  // shares of work); a workgroup whose eighth is drained helps with the next ones.
  const long nquad = (A.nray + RPW - 1) / RPW;
  const int nxcd = (gridDim.x % 8 == 0) ? 8 : 1;
  unsigned *qcnt = A.qcount + (EMIT ? 8 : 0);
  int chunk = (int)(blockIdx.x % nxcd);
  int traced = 0;
  for (;;) {
    RAYS_ARGS_FRESH;
    long quad = -1;
    if (lane == 0) {
      for (int tried = 0; tried < nxcd; tried++) {
        const long lo = nquad * chunk / nxcd, hi = nquad * (chunk + 1) / nxcd;
        const long b = lo < hi ? (long)atomicAdd(&qcnt[chunk], 1u) : hi;
        if (lo + b < hi) {
          quad = lo + b;
          break;
        }
        // (a pass beside the eikonal launch sweeps its range several times: a quad whose field was not finished when a workgroup
        // came by is offered again to the workgroups that arrive later -- no waiting, only A.sweeps cheap looks per quad)
        if (!EMIT && A.sweeps > 1 && lo < hi && b < (hi - lo) * A.sweeps) {
          quad = lo + b % (hi - lo);
          break;
        }
        chunk = (chunk + 1) % nxcd;
      }
    }
    quad = ((long)__shfl((int)(quad >> 32), 0) << 32) | (unsigned)__shfl((int)quad, 0);
    chunk = __shfl(chunk, 0);
    if (quad < 0) break;
    const long slot = quad * RPW + grp;
    if (!EMIT && A.defer_mark) {
      // Beside an asynchronous eikonal launch the count pass is a sequence of short NON-BLOCKING passes over the quads that are
      // still marked: a quad is traced (and unmarked) if the fields of all its rays are finished, left for a later pass otherwise,
      // and a workgroup leaves after max_quads of them.  A ray workgroup NEVER waits for the other kernel: waiting wavefronts were
      // seen to hold the whole chip while the eikonal launch stood still (4 071 of 4 096 ray workgroups resident and waiting, 19
      // eikonal workgroups gone, for as long as the wait was allowed to last: profiles/r6_tail_fill.md) -- which launch's
      // wavefronts are resident is the hardware scheduler's business, and nothing here may depend on it.
      if (!A.defer_mark[quad]) continue;                      // traced by an earlier pass
      if (A.fdone) {
        // (ACQUIRE: the load invalidates this XCD's cached copy of the flag -- the XCDs' L2s are not coherent with each other)
        const int fq = slot < A.nray ? A.field[A.perm ? (long)A.perm[slot] : slot] : -1;
        const int st = fq >= 0 ? __hip_atomic_load(A.fdone + fq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) : 1;
        if (__ballot(st != 1) != 0) continue;                 // a field still marching (0) or waiting for its spill rerun (2)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");    // the fields' words and refined outputs, written by another kernel on other XCDs
      }
      if (A.max_quads > 0 && traced >= A.max_quads) break;    // this pass's share is done (the quad stays marked)
      // claim the quad: a pass offers it several times, perhaps to workgroups on different XCDs, whose L2s do not see each other's
      // plain stores -- the exchange is a device-scope atomic, exactly one workgroup gets the 1
      int mine = 0;
      if (lane == 0) mine = __hip_atomic_exchange(A.defer_mark + quad, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      mine = __shfl(mine, 0);
      if (!mine) continue;
      traced++;
      if (lane == 0) atomicAdd(&A.qcount[18], 1u);
    }
    if (slot >= A.nray) continue;
    const long ray = A.perm ? (long)A.perm[slot] : slot;
    const int f = A.field[ray];
    const float scx = A.scx[f], scz = A.scz[f], rcx = A.rcx[ray], rcz = A.rcz[ray];
    const float *veln = A.veln + (size_t)(A.period[f] - 1) * nnx * nnz;
    const float *ttn = TILED ? A.ttn + (size_t)(A.tslot ? A.tslot[f] : f) * A.fstride : A.ttn + (size_t)f * nnx * nnz;
    const int tsh = TILED ? A.tsh : 0;
    // node (x0, z0), 0-based, of this field's coarse times
    auto tnode = [&](int x0, int z0) -> float {
      return TILED ? ttn[dz_tile_x(x0, tsh) + dz_tile_z(z0)] : ttn[(size_t)x0 * nnz + z0];
    };
    const float *ttnr = A.ttnr + (size_t)f * RM * RM;
    const int *nstsr = A.nstsr + (size_t)f * RM * RM;
    const dazim_refbox bx = A.boxes[f];
    const int saved = EMIT ? A.nlist[ray] : -1;   // EMIT: reuse the count pass's Frechet cells when they fit
    if (saved < 0 && gl < 4) s_rng[gl] = gl < 2 ? 0x7fffffff : -1;   // traced here: no block yet
    cbar();
    int status = 0, rb = 0;
    // ---------------- srtimes, inv/CalSurfG.f90:1644-1711 ----------------
    if (!EMIT) {
      int irx = (int)divr(rcx - gox, rdnx) + 1, irz = (int)divr(rcz - goz, rdnz) + 1;
      if (irx < 1 || irx > nnx || irz < 1 || irz > nnz) status = DAZIM_E_RECEIVER_OUTSIDE;
      if (!status) {
        if (irx == nnx) irx--;
        if (irz == nnz) irz--;
        const int isx = (int)divr(scx - gox, rdnx) + 1, isz = (int)divr(scz - goz, rdnz) + 1;
        float sred = ((scx - rcx) * EARTH) * ((scx - rcx) * EARTH);
        const float e2 = (scz - rcz) * EARTH * dz_sinf(rcx);
        sred = sqrtf(sred + e2 * e2);
        bool sw = sred < A.dplh;
        if (isx == irx && isz == irz) sw = true;
        float trr;
        if (sw) {
          const float vs = bilin_cell(g, veln, isx, isz, scx, scz, rdnx, rdnz);
          const float vr = bilin_cell(g, veln, irx, irz, rcx, rcz, rdnx, rdnz);
          trr = 2.0f * sred / (vs + vr);
        } else {
          const float drx = (rcx - gox) - (float)(irx - 1) * dnx;
          const float drz = (rcz - goz) - (float)(irz - 1) * dnz;
          trr = 0.0f;
#pragma unroll
          for (int k = 1; k <= 2; k++)
#pragma unroll
            for (int l = 1; l <= 2; l++) {
              const float produ = (1.0f - fabsf(divr((float)(l - 1) * dnz - drz, rdnz))) *
                                  (1.0f - fabsf(divr((float)(k - 1) * dnx - drx, rdnx)));
              trr = trr + tnode(irx - 2 + k, irz - 2 + l) * produ;
            }
        }
        if (gl == 0) A.dsurf[ray] = trr;
      }
    }
    // ---------------- rpaths, inv/CalSurfG.f90:1818-2236 ----------------
    const float goxr = bx.goxr, gozr = bx.gozr, dnxr = bx.dnxr, dnzr = bx.dnzr;
    const int nnxr = bx.nnxr, nnzr = bx.nnzr;
    const int isx = (int)divr(scx - goxr, rdnxr) + 1, isz = (int)divr(scz - gozr, rdnzr) + 1;
    const float dpl = 0.5f * A.dplh;
    int ipx = (int)divr(rcx - gox, rdnx) + 1, ipz = (int)divr(rcz - goz, rdnz) + 1;
    if (ipx < 1 || ipx >= nnx || ipz < 1 || ipz >= nnz) status = DAZIM_E_RECEIVER_OUTSIDE;
    if (!status && saved < 0) {
      float x0 = rcx, z0 = rcz;
      float sinx0 = dz_sinf(x0);
      int sw = 0;
      float sred = ((scx - x0) * EARTH) * ((scx - x0) * EARTH);
      float e2 = (scz - z0) * EARTH * sinx0;
      sred = sqrtf(sred + e2 * e2);
      if (sred < 2.0f * dpl) sw = 1;
      int ipxr = (int)divr(rcx - goxr, rdnxr) + 1, ipzr = (int)divr(rcz - gozr, rdnzr) + 1;
      auto in_refined = [&](int px, int pz) -> int {
        if (px < 1 || px >= nnxr || pz < 1 || pz >= nnzr) return 0;
        const int *sp = nstsr + (size_t)(px - 1) * RM + (pz - 1);
        if (sp[0] != 0 || sp[1] != 0) return 0;
        if (sp[RM] != 0 || sp[RM + 1] != 0) return 0;
        return 1;
      };
      int igref = in_refined(ipxr, ipzr);
      if (sw == 0 && igref == 1 && ipxr == isx && ipzr == isz) sw = 1;
      // ray geometry for the path files (writepath): point 1 = the receiver; a ray that ends at once gets the source as point 2
      const bool keep_pts = !EMIT && A.pts != nullptr && gl == 0;
      float2 *rp = A.pts ? A.pts + (size_t)ray * A.pcap : nullptr;
      int np = 1;
      if (keep_pts) {
        rp[0] = make_float2(rcx, rcz);
        if (sw == 1) { if (A.pcap > 1) rp[1] = make_float2(scx, scz); np = 2; }
      }
      // register-cached 4x4 block of the Frechet grid(s): this lane's cell is (bz+ll, bx+lm)
      int cbx = -100, cbz = -100;
      float acc[LPR], accc[LPR], accs[LPR];
#pragma unroll
      for (int q = 0; q < LPR; q++) acc[q] = accc[q] = accs[q] = 0.0f;
      auto flush = [&]() {
        if (cbx > -100) {
#pragma unroll
          for (int q = 0; q < LPR; q++) {
            const int fi = (cbz + l0 + q * LSTEP) * ldf + (cbx + lm);
            gfdm[fi] = acc[q];
            if (AZIM) { gfdmc[fi] = accc[q]; gfdms[fi] = accs[q]; }
          }
        }
      };
      // The corner times of the cell the NEXT step starts in are requested as soon as that cell is known (on both grids: which
      // one applies depends on node states that are still being loaded), so that they travel together with the velocity and
      // node-state loads of the current step instead of costing a second dependent round trip per step.
      float tc00, tc01, tc10, tc11, tr00 = 0.0f, tr01 = 0.0f, tr10 = 0.0f, tr11 = 0.0f;
      auto load_corner_times = [&]() {
        if (TILED) {
          const int x0 = dz_tile_x(ipx - 1, tsh), x1 = dz_tile_x(ipx, tsh), z0 = dz_tile_z(ipz - 1), z1 = dz_tile_z(ipz);
          tc00 = ttn[x0 + z0]; tc01 = ttn[x0 + z1]; tc10 = ttn[x1 + z0]; tc11 = ttn[x1 + z1];
        } else {
          const float *t = ttn + (size_t)(ipx - 1) * nnz + (ipz - 1);
          tc00 = t[0]; tc01 = t[1]; tc10 = t[nnz]; tc11 = t[nnz + 1];
        }
      };
      auto load_refined_corner_times = [&]() {
        if (ipxr >= 1 && ipxr < nnxr && ipzr >= 1 && ipzr < nnzr) {   // (outside the refined box igref is 0 and these are not used)
          const float *u = ttnr + (size_t)(ipxr - 1) * RM + (ipzr - 1);
          tr00 = u[0]; tr01 = u[1]; tr10 = u[RM]; tr11 = u[RM + 1];
        }
      };
      load_corner_times();
      load_refined_corner_times();
      // What a step needs at its starting point -- velocity and B-spline weights at (x0, z0) -- is what the step before computed at
      // its end point, bit for bit, whenever that end point was the step's (x1, z1) itself in the same cells: the last sub-segment
      // ends at x0 + 1.0f * (x1 - x0), which is x1 exactly unless the two differ by more than a factor of two (Sterbenz), and the
      // cell indices agree unless the point was clipped to the grid.  Checked per ray after every step; the values are carried
      // over only while every ray of the wavefront may (a sixth of the step's instructions otherwise repeated).
      // What is carried is the start-point term of the scatter itself, rdc = vi * wi / (vel * vel) per cell of this lane: the end-point
      // term (rdc1) of one sub-segment is the start-point term (rdc2) of the next, same operands and same operations, within a step
      // and -- with `carry` -- from the last sub-segment of one step to the first of the next.  vel, vi and wi live inside a sub-segment.
      bool carry = false;
      float rdc[LPR];
#pragma unroll
      for (int q = 0; q < LPR; q++) rdc[q] = 0.0f;
      // Wave-uniform limits of the two short cuts below, closed until the first step's start-point block (the one rare block every
      // ray passes) has looked at option rays.plain_step, and left closed by it: `fart` = +inf, no point is far from the refined box;
      // nnx_in = nnz_in = 0, no cell is interior (which also keeps `carry` off).
      // Far from the refined box: the box has at most RM nodes per axis, (RM - 1) / 8 = 16 coarse cells (eight refined cells per coarse
      // one, fmm.hip), and contains its source's cell, so a point more than 16 coarse cells from the source in x or in z is outside it.
      // One more cell of margin (eight refined cells) covers the roundings of the box origin, of the differences and of the
      // reciprocal products, which are ~1e-3 of a refined cell; max(dnx, dnz) serves both axes.  A NaN compares false: not far.
      float fart = __builtin_inff();
      int nnx_in = 0, nnz_in = 0;
      const long maxrp = (long)nnx * nnz;
      for (long j = 1; j <= maxrp; j++) {
        if (sw == 1) break;
        RAYS_MARK(0);
        float dtx, dtz;
        if (igref == 1) {
          dtx = tr10 - tr00;
          dtx = dtx + tr11 - tr01;
          dtx = divr(dtx, A.r_e2dnxr);
          dtz = tr01 - tr00;
          dtz = dtz + tr11 - tr10;
          dtz = dtz / (2.0f * EARTH * sinx0 * dnzr);
        } else {
          dtx = tc10 - tc00;
          dtx = dtx + tc11 - tc01;
          dtx = divr(dtx, A.r_e2dnx);
          dtz = tc01 - tc00;
          dtz = dtz + tc11 - tc10;
          dtz = dtz / (2.0f * EARTH * sinx0 * dnz);
        }
        const float rd1 = sqrtf(dtx * dtx + dtz * dtz);
        float x1 = x0 - dpl * dtx / (EARTH * rd1);
        float z1 = z0 - dpl * dtz / (EARTH * sinx0 * rd1);
        RAYS_MARK(1);
        const int ipxo = ipx, ipzo = ipz;
        const float sdx = scx - x1, sdz = scz - z1;
        bool srcell = false;   // the point is in the source's cell of the refined grid
        if (__ballot(!(fabsf(sdx) > fart || fabsf(sdz) > fart)) != 0) {
          ipxr = (int)divr(x1 - goxr, rdnxr) + 1;
          ipzr = (int)divr(z1 - gozr, rdnzr) + 1;
          igref = in_refined(ipxr, ipzr);
          srcell = igref == 1 && ipxr == isx && ipzr == isz;
          load_refined_corner_times();
        } else {   // every ray of the wavefront is far from its refined box: in_refined would be 0 and the refined times unused
          igref = 0;
        }
        ipx = (int)divr(x1 - gox, rdnx) + 1;
        ipz = (int)divr(z1 - goz, rdnz) + 1;
        RAYS_MARK(2);
        float sinx1 = dz_sinf(x1);
        sred = (sdx * EARTH) * (sdx * EARTH);
        e2 = sdz * EARTH * sinx1;
        sred = sqrtf(sred + e2 * e2);
        sw = 0;
        if (sred < 2.0f * dpl) sw = 1;
        if (srcell) sw = 1;
        RAYS_MARK(3);
        bool clipx = false;
        if (ipx < 1) { x1 = gox; ipx = 1; rb = 1; clipx = true; }
        if (ipx >= nnx) { x1 = gox + (float)(nnx - 1) * dnx; ipx = nnx - 1; rb = 1; clipx = true; }
        if (ipz < 1) { z1 = goz; ipz = 1; rb = 1; }
        if (ipz >= nnz) { z1 = goz + (float)(nnz - 1) * dnz; ipz = nnz - 1; rb = 1; }
        RAYS_MARK(4);
        load_corner_times();
        if (keep_pts) {   // rgx(j+1) after the clipping, then rgx(j+2) = the source if this was the last step (:352-400)
          if (np < A.pcap) rp[np] = make_float2(x1, z1);
          np++;
          if (sw == 1) {
            if (np < A.pcap) rp[np] = make_float2(scx, scz);
            np++;
          }
        }
        if (clipx) sinx1 = dz_sinf(x1);   // the next step starts from the clipped point
        float c2psi = 0.0f, s2psi = 0.0f;
        if (AZIM) step_azimuth(x0, z0, x1, z1, c2psi, s2psi);
        RAYS_MARK(5);
        // ---- Frechet weights, :2077-2229 ----
        const int ivx = (ipx - 1) / GDX + 1, ivz = (ipz - 1) / GDZ + 1;
        const int ivxo = (ipxo - 1) / GDX + 1, ivzo = (ipzo - 1) / GDZ + 1;
        int nhp = 0, chp0 = 0, chp1 = 0;
        float vr0 = 1.0f, vr1 = 1.0f, vr2 = 1.0f;
        if (ivx != ivxo) {
          nhp = 1;
          const float xi = (ivx > ivxo) ? gox + (float)(ivx - 1) * dvx : gox + (float)ivx * dvx;
          vr0 = (xi - x0) / (x1 - x0);
          chp0 = 1;
        }
        if (ivz != ivzo) {
          const float zi = (ivz > ivzo) ? goz + (float)(ivz - 1) * dvz : goz + (float)ivz * dvz;
          const float r = (zi - z0) / (z1 - z0);
          if (nhp == 0) {
            vr0 = r;
            chp0 = 2;
          } else if (r >= vr0) {
            vr1 = r;
            chp1 = 2;
          } else {
            vr1 = vr0;
            chp1 = chp0;
            vr0 = r;
            chp0 = 2;
          }
          nhp++;
        }
        nhp++;  // the closing sub-segment with vrat = 1, chp = 0
        if (nhp == 1) vr0 = 1.0f;
        if (nhp == 2) vr1 = 1.0f;
        RAYS_MARK(6);
        float drx, drz;
        if (__builtin_expect(__ballot(!carry) != 0, 0)) {  // (first step, clipped points: rare -- and wave-uniform, so out of line)
          drx = (x0 - gox) - (float)(ipxo - 1) * dnx;
          drz = (z0 - goz) - (float)(ipzo - 1) * dnz;
          const float vel = vel_at(g, veln, ipxo, ipzo, drx, drz, rdnx, rdnz);
          drx = (x0 - gox) - (float)(ivxo - 1) * dvx;
          drz = (z0 - goz) - (float)(ivzo - 1) * dvz;
          const float vi = basis1(divr(drx, rdvx), lm);
#pragma unroll
          for (int q = 0; q < LPR; q++) rdc[q] = vi * basis1(divr(drz, rdvz), l0 + q * LSTEP) / (vel * vel);
          if (A.plain_step == 0) {   // open the short cuts (see above)
            fart = (float)((RM - 1) / 8 + 1) * fmaxf(dnx, dnz);
            nnx_in = nnx;
            nnz_in = nnz;
          }
        }
        RAYS_MARK(7);
        int ivxt = ivxo, ivzt = ivzo;
        bool endsame = false;
        for (int k = 1; k <= nhp; k++) {
          if (k > 1) {
            const int cp = (k == 2) ? chp0 : chp1;
            if (cp == 1) ivxt = ivx;
            else if (cp == 2) ivzt = ivz;
          }
          const float vrk = (k == 1) ? vr0 : (k == 2 ? vr1 : vr2);
          const float vrp = (k == 2) ? vr0 : vr1;
          const float rigz = z0 + vrk * (z1 - z0);
          const float rigx = x0 + vrk * (x1 - x0);
          const int ipxt = (int)divr(rigx - gox, rdnx) + 1, ipzt = (int)divr(rigz - goz, rdnz) + 1;
          endsame = rigx == x1 && rigz == z1 && ipxt == ipx && ipzt == ipz && ivxt == ivx && ivzt == ivz;   // (of the last sub-segment)
          drx = (rigx - gox) - (float)(ipxt - 1) * dnx;
          drz = (rigz - goz) - (float)(ipzt - 1) * dnz;
          const bool inner = ipxt >= 1 && ipxt < nnx_in && ipzt >= 1 && ipzt < nnz_in;
          endsame = endsame && inner;   // (a start point in an edge cell is formed anew by the general vel_at)
          float vel;
          if (__builtin_expect(__ballot(!inner) == 0, 1)) vel = vel_at_interior(g, veln, ipxt, ipzt, drx, drz, rdnx, rdnz);
          else vel = vel_at(g, veln, ipxt, ipzt, drx, drz, rdnx, rdnz);
          drx = (rigx - gox) - (float)(ivxt - 1) * dvx;
          drz = (rigz - goz) - (float)(ivzt - 1) * dvz;
          const float vi = basis1(divr(drx, rdvx), lm);
          float wi[LPR];            // this lane's vi(m), wi(l)
#pragma unroll
          for (int q = 0; q < LPR; q++) wi[q] = basis1(divr(drz, rdvz), l0 + q * LSTEP);
          const float dinc = (k == 1) ? vrk * dpl : (vrk - vrp) * dpl;
          // block of this sub-segment: cells (ivzt-2+l, ivxt-2+m), l,m = 1..4
          const int nbx = ivxt - 1, nbz = ivzt - 1;
          RAYS_MARK(8);
          if (nbx != cbx || nbz != cbz) {
            flush();
            cbar();
            cbx = nbx;
            cbz = nbz;
            // (LDS atomics without a result: no register, and the lanes of a group all bring the same values)
            __hip_atomic_fetch_min(s_rng + 0, nbx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(s_rng + 1, nbz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(s_rng + 2, nbx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(s_rng + 3, nbz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
            for (int q = 0; q < LPR; q++) {
              const int fi = (cbz + l0 + q * LSTEP) * ldf + (cbx + lm);
              acc[q] = gfdm[fi];
              if (AZIM) { accc[q] = gfdmc[fi]; accs[q] = gfdms[fi]; }
            }
          }
          RAYS_MARK(9);
#pragma unroll
          for (int q = 0; q < LPR; q++) {
            const float rdc1 = vi * wi[q] / (vel * vel);
            const float rdc2 = rdc[q];
            rdc[q] = rdc1;
            float r1 = -(rdc1 + rdc2) * dinc / 2.0f;
            acc[q] = r1 + acc[q];
            if (AZIM) {   // inv/rpathsAzim.f90:580-586
              r1 = -(rdc1 * c2psi + rdc2 * c2psi) * dinc / 2.0f;
              accc[q] = r1 + accc[q];
              r1 = -(rdc1 * s2psi + rdc2 * s2psi) * dinc / 2.0f;
              accs[q] = r1 + accs[q];
            }
          }
        }
        RAYS_MARK(10);
        carry = endsame;
        x0 = x1;
        z0 = z1;
        sinx0 = sinx1;
      RAYS_MARK(11);
      }
      flush();
      if (keep_pts) A.npts[ray] = np <= A.pcap ? np : -1;
    }
    cbar();
    if (!EMIT && gl == 0) {
      if (A.pts && status) A.npts[ray] = 0;
      A.status[ray] = status;
      A.rbflag[ray] = rb;
    }
    // ---------------- G row, inv/CalSurfG.f90:1339-1364 ----------------
    // cells with |fdm| >= ftol in (jj,kk) order -> this group's LDS list
    // The usual ray (its cell list fits RC cells per lane, the combined kernels are there, no dense twin) takes the register form of
    // the row assembly below; a saved list of that kind is read where it lies (A.lval) and the slot is not touched.
    auto usual = [&](int n) { return n <= LC && n <= RC * GP && (MAP || A.skern != nullptr) && !A.dense; };
    int nlist = 0;
    if (saved >= 0) {
      nlist = saved;
      const size_t o = (size_t)ray * A.LK, ov = o * NG;
      const bool viaslot = !usual(saved);   // (the general loop reads the slot: cleared again at the end of the ray)
      for (int i = gl; i < nlist; i += GP) {
        const int c = A.lcell[o + i];
        s_list[i] = (unsigned short)c;
        if (viaslot) {
          const int jj = (int)__umulhi((unsigned)c, nvx_magic) + 1, kk = c - (jj - 1) * nvx + 1;
          gfdm[jj * ldf + kk] = A.lval[ov + i];
          if (AZIM) {
            gfdmc[jj * ldf + kk] = A.lval[ov + A.LK + i];
            gfdms[jj * ldf + kk] = A.lval[ov + 2 * A.LK + i];
          }
        }
      }
    } else if (!status) {
      // the rows and columns of the blocks the ray has been in, in ascending cell order (everything else is zero, below FTOL);
      // no block at all: an empty range
      const int kk0 = max(s_rng[0], 1), kk1 = min(s_rng[2] + 3, nvx), jj0 = max(s_rng[1], 1), jj1 = min(s_rng[3] + 3, nvz);
      for (int jj = jj0; jj <= jj1; jj++)
        for (int kb = kk0; kb <= kk1; kb += GP) {
          const int kk = kb + gl;
          const bool keep = kk <= kk1 && fabsf(gfdm[jj * ldf + kk]) >= FTOL;
          const unsigned m = (unsigned)((__ballot(keep) >> gmask_shift) & GMASK);
          const int pos = nlist + __popc(m & ((1u << gl) - 1u));
          if (keep && pos < LC) s_list[pos] = (unsigned short)((jj - 1) * nvx + kk - 1);
          nlist += __popc(m);
        }
    }
    cbar();
    if (!EMIT) {   // hand the Frechet cells to the emit pass so that it need not trace the ray again
      const size_t o = (size_t)ray * A.LK, ov = o * NG;
      if (nlist <= A.LK)
        for (int i = gl; i < nlist; i += GP) {
          const int c = s_list[i];
          const int jj = (int)__umulhi((unsigned)c, nvx_magic) + 1, kk = c - (jj - 1) * nvx + 1;
          A.lcell[o + i] = (unsigned short)c;
          A.lval[ov + i] = gfdm[jj * ldf + kk];
          if (AZIM) {
            A.lval[ov + A.LK + i] = gfdmc[jj * ldf + kk];
            A.lval[ov + 2 * A.LK + i] = gfdms[jj * ldf + kk];
          }
        }
      if (gl == 0) A.nlist[ray] = (status || nlist <= A.LK) ? (status ? 0 : nlist) : -1;
    }
    const size_t ncol = (size_t)A.nx * A.ny;
    const int kslot = A.kidx[f] - 1;
    long cnt = 0;
    const long rstart = EMIT ? A.rowptr[ray] : 0;
    const int nparpi = nvx * nvz * (A.nz - 1);
    // column blocks: dVs | Gc | Gs of nparpi columns each, or (MAP) c | a1 | a2 of kmax maps each, this field's map at poff
    const int nlay = MAP ? 1 : A.nz - 1;
    const int bstride = MAP ? A.kmax * nvx * nvz : nparpi;
    const int poff = MAP ? (A.period[f] - 1) * nvx * nvz : 0;
    const bool lovf = nlist > LC;                       // list did not fit: sweep the whole grid instead (rare)
    const int ntot = lovf ? nvz * nvx : nlist;
    long cntd = 0;
    int jjL = 1, kkL = 1;                               // dense twin: the last cell with |fdm| >= ftol in (jj, kk) order
    if (A.dense) {
      int clast = -1;
      if (!lovf) {
        if (nlist > 0) clast = s_list[nlist - 1];
      } else {
        for (int base = ((nvz * nvx - 1) / GP) * GP; base >= 0 && clast < 0; base -= GP) {
          const int c = base + gl;
          bool k2 = false;
          if (c < nvz * nvx) {
            const int jj = (int)__umulhi((unsigned)c, nvx_magic) + 1, kk = c - (jj - 1) * nvx + 1;
            k2 = fabsf(gfdm[jj * ldf + kk]) >= FTOL;
          }
          const unsigned m2 = (unsigned)((__ballot(k2) >> gmask_shift) & GMASK);
          if (m2) clast = base + (31 - __clz(m2));
        }
      }
      if (clast >= 0) { jjL = (int)__umulhi((unsigned)clast, nvx_magic) + 1; kkL = clast - (jjL - 1) * nvx + 1; }
    }
    // The usual ray (its cell list fits RC cells per lane, the combined kernels are there, no dense twin): every cell's indices and
    // Frechet values are decoded and loaded ONCE into registers and the layers loop over them, where the general loop below decodes
    // the cell id and reloads its Frechet value for each of the nz - 1 layers.  Same entries in the same order.
    // (RC = 8: 128 cells in the emit pass, where a ray of the S-256 batch has ~100; 64 in the count pass: sixteen per lane there cost the tracing loop registers, 38.1 -> 40.1 ms)
    const bool rowcache = usual(nlist);
    if (rowcache) {
      int sidx[RC], cbase[RC], fidx[RC];
#pragma unroll
      for (int i = 0; i < RC; i++) {
        const int li = i * GP + gl;
        const int c = li < ntot ? (int)s_list[li] : 0;
        const int jj = (int)__umulhi((unsigned)c, nvx_magic) + 1, kk = c - (jj - 1) * nvx + 1;
        sidx[i] = jj * (nvx + 2) + kk;
        cbase[i] = (jj - 1) * nvx + kk;
        fidx[i] = jj * ldf + kk;
      }
      for (int blk = 0; blk < NG; blk++) {
        float fdv[RC];
        const float *fsrc = blk == 0 ? gfdm : (blk == 1 ? gfdmc : gfdms);
        const float *lsrc = A.lval + ((size_t)ray * NG + blk) * A.LK;   // a saved list: the same bits, contiguous
#pragma unroll
        for (int i = 0; i < RC; i++) fdv[i] = (i * GP + gl < ntot) ? (saved >= 0 ? lsrc[i * GP + gl] : fsrc[fidx[i]]) : 0.0f;
        for (int k = 1; k <= nlay; k++) {
          const size_t sk = ((size_t)(k - 1) * A.kmax + kslot) * ncol;
          const int nk = blk * bstride + poff + (k - 1) * nvz * nvx;
#pragma unroll
          for (int i = 0; i < RC; i++) {
            if (i * GP >= ntot) break;                    // (per ray: the lanes of a group leave together)
            const bool cell = i * GP + gl < ntot;
            float rowv = 0.0f;
            bool keep = false;
            if (cell) {
              if (MAP) rowv = fdv[i];                     // (= (float)(1.0 * (double)fdv) and 1.0f * fdv of the unit kernels)
              else if (blk == 0) rowv = (float)(A.skern[sk + sidx[i]] * (double)fdv[i]);
              else rowv = A.lsen[sk + sidx[i]] * fdv[i];
              keep = A.keep_small ? (rowv != 0.0f) : (fabsf(rowv) > FTOL);
            }
            const unsigned m = (unsigned)((__ballot(keep) >> gmask_shift) & GMASK);
            if (EMIT && keep) {
              const long pos = rstart + cnt + __popc(m & ((1u << gl) - 1u));
              A.val[pos] = rowv;
              A.col[pos] = nk + cbase[i] - 1;
            }
            cnt += __popc(m);
          }
        }
      }
    } else
    for (int blk = 0; blk < NG; blk++)   // dVs | Gc | Gs column blocks (inv/CalSurfGAniso_Joint.f90:728-738)
      for (int k = 1; k <= nlay; k++) {
        for (int base = 0; base < ntot; base += GP) {
          const int li = base + gl;
          bool keep = false, keepd = false;
          float rowv = 0.0f;
          int nn = 0;
          bool cell = li < ntot;
          int c = 0;
          if (cell) c = lovf ? li : s_list[li];
          const int jj = (int)__umulhi((unsigned)c, nvx_magic) + 1, kk = c - (jj - 1) * nvx + 1;
          if (cell && lovf) cell = fabsf(gfdm[jj * ldf + kk]) >= FTOL;
          if (cell && MAP) {
            rowv = (blk == 0 ? gfdm : (blk == 1 ? gfdmc : gfdms))[jj * ldf + kk];
            keep = A.keep_small ? (rowv != 0.0f) : (fabsf(rowv) > FTOL);
            nn = blk * bstride + poff + (jj - 1) * nvx + kk;
          } else if (cell) {
            const size_t si = ((size_t)(k - 1) * A.kmax + kslot) * ncol + (size_t)jj * (nvx + 2) + kk;
            if (blk == 0) {
              const float fd = gfdm[jj * ldf + kk];
              double r;
              if (A.skern) {
                r = A.skern[si] * (double)fd;           // (the cell's factor from k_row_kernels: same operations, same order)
              } else {
                const float v = A.vels[((size_t)(k - 1) * A.ny + jj) * A.nx + kk];
                const float coe_a = (2.0947f - 0.8206f * 2 * v + 0.2683f * 3 * (v * v) - 0.0251f * 4 * (v * v * v));
                const float vpft = 0.9409f + 2.0947f * v - 0.8206f * (v * v) + 0.2683f * (v * v * v) - 0.0251f * (v * v * v * v);
                const float coe_rho = coe_a * (1.6612f - 0.4721f * 2 * vpft + 0.0671f * 3 * (vpft * vpft) -
                                               0.0043f * 4 * (vpft * vpft * vpft) + 0.000106f * 5 * (vpft * vpft * vpft * vpft));
                r = (A.svp[si] * (double)coe_a + A.srho[si] * (double)coe_rho + A.svs[si]) * (double)fd;
              }
              rowv = (float)r;
              if (A.dense) {   // the same expression with the derivatives left over from the last cell of the first loop
                const float vL = A.vels[((size_t)(k - 1) * A.ny + jjL) * A.nx + kkL];
                const float caL = (2.0947f - 0.8206f * 2 * vL + 0.2683f * 3 * (vL * vL) - 0.0251f * 4 * (vL * vL * vL));
                const float vpL = 0.9409f + 2.0947f * vL - 0.8206f * (vL * vL) + 0.2683f * (vL * vL * vL) - 0.0251f * (vL * vL * vL * vL);
                const float crL = caL * (1.6612f - 0.4721f * 2 * vpL + 0.0671f * 3 * (vpL * vpL) -
                                         0.0043f * 4 * (vpL * vpL * vpL) + 0.000106f * 5 * (vpL * vpL * vpL * vpL));
                const double rd = (A.svp[si] * (double)caL + A.srho[si] * (double)crL + A.svs[si]) * (double)fd;
                keepd = (float)rd != 0.0f;
                if (EMIT && A.dense == 1) rowv = (float)rd;
              }
            } else {
              rowv = A.lsen[si] * (blk == 1 ? gfdmc : gfdms)[jj * ldf + kk];
              keepd = rowv != 0.0f;
            }
            keep = A.keep_small ? (rowv != 0.0f) : (fabsf(rowv) > FTOL);
            if (EMIT && A.dense == 1) keep = keepd;
            nn = blk * bstride + (k - 1) * nvz * nvx + (jj - 1) * nvx + kk;  // 1-based column of the reference
          }
          if (!EMIT && A.dense == 2) cntd += __popc((unsigned)((__ballot(keepd) >> gmask_shift) & GMASK));
          const unsigned m = (unsigned)((__ballot(keep) >> gmask_shift) & GMASK);
          if (EMIT && keep) {
            const long pos = rstart + cnt + __popc(m & ((1u << gl) - 1u));
            A.val[pos] = rowv;
            A.col[pos] = nn - 1;
          }
          cnt += __popc(m);
        }
      }
    // zeros back into what this ray wrote, so that the slot's next ray finds it clean: the rectangle of its blocks (border rows and
    // columns included; empty for a ray with a status, which traced nothing), or the cells of a saved list that went through the slot
    cbar();
    if (saved < 0) {
      const int x0 = max(s_rng[0], 0), x1 = min(s_rng[2] + 3, nvx + 1), z0 = max(s_rng[1], 0), z1 = min(s_rng[3] + 3, nvz + 1);
      for (int z = z0; z <= z1; z++)
        for (int x = x0 + gl; x <= x1; x += GP) {
          gfdm[z * ldf + x] = 0.0f;
          if (AZIM) { gfdmc[z * ldf + x] = 0.0f; gfdms[z * ldf + x] = 0.0f; }
        }
    } else if (!rowcache) {
      for (int i = gl; i < nlist; i += GP) {
        const int c = s_list[i];
        const int jj = (int)__umulhi((unsigned)c, nvx_magic) + 1, kk = c - (jj - 1) * nvx + 1;
        gfdm[jj * ldf + kk] = 0.0f;
        if (AZIM) { gfdmc[jj * ldf + kk] = 0.0f; gfdms[jj * ldf + kk] = 0.0f; }
      }
    }
    cbar();
    if (!EMIT && gl == 0) {
      A.count[ray] = cnt;
      if (A.dense == 2) A.countd[ray] = cntd;
      if (lovf) atomicAdd(&A.qcount[16], 1u);           // (statistics only: dazim_last_kernel_seconds("rays.list_sweeps"))
      if (!status && nlist > A.LK) atomicAdd(&A.qcount[17], 1u);
    }
  }
}
#undef A
#undef RAYS_ARGS_FRESH

// One dazim_rays_build_G* call on the host: the entry's arguments by name, what the stages hand each other, and a member function
// per stage (run() is the order).  Members are destroyed in reverse order, so on every early return the matrix arrays go back to
// the cache first, then the staged inputs, then the third stream is drained and the context's stream restored.
struct RayBuild {
  // ---- the call ----
  dazim_ctx *ctx;
  int nx = 0, ny = 0, nz = 0, kmax = 0, nfield = 0;
  float goxd = 0, gozd = 0, dvxd = 0, dvzd = 0;
  const float *vels = nullptr, *scx = nullptr, *scz = nullptr, *veln = nullptr, *ttn = nullptr, *ttnr = nullptr, *rcx = nullptr, *rcz = nullptr;
  const float *lsen = nullptr;   // joint rows (3-D)
  const int *period = nullptr, *kidx = nullptr, *nstsr = nullptr, *field = nullptr;
  const dazim_refbox *boxes = nullptr;
  const double *svs = nullptr, *svp = nullptr, *srho = nullptr;
  int64_t nray = 0;
  float *dsurf = nullptr;   // outputs
  dazim_csr **G = nullptr;
  int64_t *nnz_out = nullptr;
  int *n_boundary = nullptr;
  bool map = false, azim = false;   // map rows (dazim_rays_build_G_maps), with the 2-psi blocks
  // ---- guards ----
  struct StreamSwap {   // while the count pass is prepared and launched, "the context's stream" is the third stream
    dazim_ctx *c; hipStream_t main; bool on = false;
    void restore() { if (on) { c->stream = main; on = false; } }
    ~StreamSwap() {
      if (on) (void)hipStreamSynchronize(c->stream);   // (an early return: nothing of this call may still run when its buffers go)
      restore();
    }
  } swap;
  struct {
    DzBuf<float> vels, scx, scz, veln, ttn, ttnr, rcx, rcz, dsurf, lsen;
    DzBuf<int> period, kidx, nstsr, field;
    DzBuf<dazim_refbox> boxes;
    DzBuf<double> svs, svp, srho;
  } d;
  struct Arrays {   // the matrix arrays go back to the cache on every early return (until the matrix has adopted them)
    dazim_ctx *c; int64_t *rp = nullptr; float *v = nullptr; int *cl = nullptr; int64_t nnz = 0, cap_nnz = 0; bool keep = false;
    ~Arrays() { if (!keep) { dz_big_put(c, rp); dz_big_put(c, v); dz_big_put(c, cl); } }
  } arrays, arrays_d;   // G and its dense twin
  // ---- between the stages ----
  dazim_geom g;
  bool joint = false, tiled = false, overlap = false, twin = false;
  size_t nn = 0, nr = 0, ncol = 0, nk = 0, nr1 = 0, lds = 0;
  int64_t res_rows = 0, res_nnz = 0;
  long nwg = 0;
  double overlap_tail_s = 0.0;
  RayArgs A;
  explicit RayBuild(dazim_ctx *c) : ctx(c), swap{c, c ? c->stream : nullptr}, arrays{c}, arrays_d{c} {}
  int check() {
    if (!ctx || !G) return DAZIM_E_BAD_ARG;
    // map mode (dazim_rays_build_G_maps): no model, no depth kernels; nz = 2 stands for the one "layer" of a map
    joint = map ? azim : lsen != nullptr;
    if (map) nz = 2;
    if (map && dz_opt(ctx, "rays.dense_twin", 0) != 0)
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_rays_build_G_maps: option rays.dense_twin serves the 3-D program's diagnostics only");
    if (dazim_geometry(nx, ny, goxd, gozd, dvxd, dvzd, &g)) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad grid");
    if (nray < 0 || nfield < 1 || nz < 2 || kmax < 1 || (size_t)g.nvx * g.nvz > 65535u) return dz_fail(ctx, DAZIM_E_BAD_ARG, "bad arguments to dazim_rays_build_G");
    // every array the kernels dereference must be there: dazim_fmm_batch can be called without the refined outputs (ttnr, nstsr,
    // boxes nullable there), but the ray tracer reads them next to the source (inv/CalSurfG.f90:1941-1952)
    // ttn == NULL: the coarse fields are the ones the last dazim_fmm_batch call (made with ttn == NULL) kept inside the library
    tiled = ttn == nullptr;
    if (tiled && (!ctx->fields.tiled || ctx->fields.nfield != nfield || ctx->fields.nnx != g.nnx || ctx->fields.nnz != g.nnz))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_rays_build_G: ttn is NULL and the last dazim_fmm_batch call did not keep %d fields of this grid inside the library (call it with ttn = NULL)", nfield);
    if (!scx || !scz || !period || !veln || !ttnr || !nstsr || !boxes || !dsurf ||
        (!map && (!vels || !svs || !svp || !srho)) || (nray > 0 && (!field || !rcx || !rcz)))
      return dz_fail(ctx, DAZIM_E_BAD_ARG, "dazim_rays_build_G: NULL array (the refined fields ttnr, nstsr and boxes of dazim_fmm_batch are required)");
    DZ_HIP(hipSetDevice(ctx->device));
    return 0;
  }
  int decide_overlap() {
    // An asynchronous eikonal call (option fmm.async) is still marching: the count pass goes to the context's third stream, where its
    // workgroups are dispatched as the eikonal launch's persistent workgroups leave and every quad of rays waits for its fields'
    // completion flags -- the ray kernel fills the tail of the eikonal launch.  Only if nothing here has to wait on the host for the
    // main stream (every array device-resident); otherwise the eikonal call is completed first.
    overlap = (bool)ctx->fmm_finish && tiled && ctx->fields.fdone && nray > 0;
    // (a pending gather of sharded dispersion tables would run on the third stream too -- dz_join_aux below --: fine with the file
    // transport, whose collectives are host-staged; an RCCL communicator is kept to ONE stream, the main one, so with RCCL the
    // eikonal call is completed first.)
    if (overlap && ctx->aux_epilogue && ctx->comm && ((DzComm *)ctx->comm)->nccl) overlap = false;
    if (overlap)
      for (const void *q : {(const void *)vels, (const void *)scx, (const void *)scz, (const void *)period, (const void *)veln,
                            (const void *)ttnr, (const void *)nstsr, (const void *)boxes, (const void *)field, (const void *)rcx,
                            (const void *)rcz, (const void *)svs, (const void *)svp, (const void *)srho, (const void *)dsurf,
                            (const void *)kidx, (const void *)lsen})
        if (q && !dz_is_device_ptr(q)) overlap = false;
    if (!overlap) { const int rcf = dz_fmm_finish(ctx); if (rcf) return rcf; }
    if (overlap) {
      DZ_HIP(hipStreamWaitEvent(ctx->stream3, ctx->ev_pre, 0));   // the velocity grids and the cleared flags, enqueued before the launch
      ctx->stream = ctx->stream3;
      swap.on = true;
    }
    // the depth kernels may still be in the making on the auxiliary stream (dazim_dispersion_kernels with disp.async)
    return dz_join_aux(ctx);
  }
  int stage_inputs() {
    nn = (size_t)g.nnx * g.nnz; nr = (size_t)RM * RM; ncol = (size_t)nx * ny;
    int rc;
    if (!map && (rc = d.vels.init(ctx, vels, (size_t)nz * ncol, true, false))) return rc;
    if ((rc = d.scx.init(ctx, scx, nfield, true, false)) || (rc = d.scz.init(ctx, scz, nfield, true, false)) ||
        (rc = d.period.init(ctx, period, nfield, true, false)) || (rc = d.kidx.init(ctx, kidx ? kidx : period, nfield, true, false)) ||
        (rc = d.veln.init(ctx, veln, nn * kmax, true, false)) || (!tiled && (rc = d.ttn.init(ctx, ttn, nn * nfield, true, false))) ||
        (rc = d.ttnr.init(ctx, ttnr, nr * nfield, true, false)) || (rc = d.nstsr.init(ctx, nstsr, nr * nfield, true, false)) ||
        (rc = d.boxes.init(ctx, boxes, nfield, true, false)) || (rc = d.field.init(ctx, field, nray, true, false)) ||
        (rc = d.rcx.init(ctx, rcx, nray, true, false)) || (rc = d.rcz.init(ctx, rcz, nray, true, false)))
      return rc;
    nk = (size_t)nz * kmax * ncol;
    if (!map && ((rc = d.svs.init(ctx, svs, nk, true, false)) || (rc = d.svp.init(ctx, svp, nk, true, false)) ||
                  (rc = d.srho.init(ctx, srho, nk, true, false))))
      return rc;
    if ((rc = d.dsurf.init(ctx, dsurf, nray, false, true))) return rc;
    if (joint && !map && (rc = d.lsen.init(ctx, lsen, (size_t)(nz - 1) * kmax * ncol, true, false))) return rc;
    // index conventions follow the reference: periods and kernel slots 1-based (periods(srcnum,knumi), knumi), field_of_ray 0-based
    if ((rc = dz_check_range(ctx, d.period.dev, nfield, 1, kmax, "period_idx"))) return rc;
    if ((rc = dz_check_range(ctx, d.kidx.dev, nfield, 1, kmax, "kernel_idx"))) return rc;
    return dz_check_range(ctx, d.field.dev, nray, 0, nfield - 1, "field_of_ray");
  }
  int kernel_constants() {
    int rc;
    A.g = g;
    A.nx = nx; A.ny = ny; A.nz = nz; A.kmax = kmax;
    A.nray = nray;
    A.field = d.field.dev; A.rcx = d.rcx.dev; A.rcz = d.rcz.dev; A.scx = d.scx.dev; A.scz = d.scz.dev;
    A.period = d.period.dev; A.kidx = d.kidx.dev; A.veln = d.veln.dev; A.ttn = d.ttn.dev; A.ttnr = d.ttnr.dev;
    A.tslot = nullptr; A.tsh = 0; A.fstride = (long)nn;
    if (tiled) {
      A.ttn = reinterpret_cast<const float *>(ctx->fields.tiled);   // (the node word of a finished node is its time)
      A.tslot = ctx->fields.tslot; A.tsh = ctx->fields.tsh; A.fstride = ctx->fields.stride;
    }
    ctx->ksec["rays.tiled_fields"] = tiled ? 1.0 : 0.0;
    ctx->ksec["rays.map"] = map ? 1.0 : 0.0;
    ctx->ksec["rays.overlap"] = overlap ? 1.0 : 0.0;
    A.fdone = overlap ? ctx->fields.fdone : nullptr;
    A.defer_mark = nullptr; A.max_quads = 0; A.sweeps = 1;
    A.nstsr = d.nstsr.dev; A.boxes = d.boxes.dev; A.vels = d.vels.dev; A.svs = d.svs.dev; A.svp = d.svp.dev; A.srho = d.srho.dev;
    A.lsen = joint && !map ? d.lsen.dev : nullptr;
    A.skern = nullptr;
    {
      const unsigned dv = (unsigned)g.nvx;
      A.nvx_magic = (unsigned)((0x100000000ull + dv - 1) / dv);
      for (unsigned c = 0; c < 65536u; c++)   // (cell ids are 16-bit: the identity is checked for all of them, once per call)
        if ((unsigned)(((unsigned long long)c * A.nvx_magic) >> 32) != c / dv) return dz_fail(ctx, DAZIM_E_BAD_ARG, "internal: reciprocal of nvx");
    }
    if (!map && dz_opt(ctx, "rays.skern", 1) != 0) {   // (option rays.skern = 0: every entry from the three kernels)
      double *pk;
      if ((rc = dz_scratch(ctx, "rays.skern", nk, &pk))) return rc;
      hipLaunchKernelGGL(k_row_kernels, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, ctx->stream, (long)nk, kmax, (long)ncol,
                         d.vels.dev, d.svs.dev, d.svp.dev, d.srho.dev, pk);
      DZ_HIP(hipGetLastError());
      A.skern = pk;
    }
    {  // dpl, inv/CalSurfG.f90:1829-1833 (host libm sin, geometry only)
      float dpl = g.dnx * EARTH;
      float rd1 = g.dnz * EARTH * sinf(g.gox);
      if (rd1 < dpl) dpl = rd1;
      rd1 = g.dnz * EARTH * sinf(g.gox + (float)(g.nnx - 1) * g.dnx);
      if (rd1 < dpl) dpl = rd1;
      A.dplh = dpl;
    }
    {  // reciprocals of the loop-invariant divisors of the ray kernel (divr): the divisors as fp32 values the kernel would divide by
      const float dnxr = g.dvx / (float)(GDX * 8), dnzr = g.dvz / (float)(GDZ * 8);   // = dazim_refbox::dnxr/dnzr (sgdl = 8, fmm.hip)
      const float e2dnx = 2.0f * EARTH * g.dnx, e2dnxr = 2.0f * EARTH * dnxr;
      A.r_dnx = 1.0 / (double)g.dnx;   A.r_dnz = 1.0 / (double)g.dnz;
      A.r_dnxr = 1.0 / (double)dnxr;   A.r_dnzr = 1.0 / (double)dnzr;
      A.r_dvx = 1.0 / (double)g.dvx;   A.r_dvz = 1.0 / (double)g.dvz;
      A.r_e2dnx = 1.0 / (double)e2dnx; A.r_e2dnxr = 1.0 / (double)e2dnxr;
    }
    return 0;
  }
  int scratch() {
    int rc;
    nr1 = (size_t)(nray > 0 ? nray : 1);
    if ((rc = dz_scratch(ctx, "rays.status", nr1, &A.status))) return rc;
    if ((rc = dz_scratch(ctx, "rays.rb", nr1, &A.rbflag))) return rc;
    if ((rc = dz_scratch(ctx, "rays.count", (size_t)(nray + 1), &A.count))) return rc;
    // LDS cell lists: 512 entries keep 16 wavefronts (128 rays) on a CU, which is worth 25 % on the S-256 grid where longer lists
    // are rare; large inversion grids (S-512: rays cross > 100 cells) get 1024.  Longer lists fall back to a full-grid sweep.
    A.lcap = g.nvx * g.nvz <= 4096 ? 512 : 1024;
    if (dz_opt(ctx, "rays.lcap", 0) >= 16 && dz_opt(ctx, "rays.lcap", 0) <= 8192) A.lcap = dz_opt(ctx, "rays.lcap", 0);   // tuning / test knob: small values force the fallbacks
    if (A.lcap > g.nvx * g.nvz) A.lcap = g.nvx * g.nvz;
    A.LK = A.lcap;   // cell lists handed from the count pass to the emit pass (longer ones are traced again)
    A.keep_small = dz_opt(ctx, "rays.keep_small", 0) != 0 ? 1 : 0;
    A.plain_step = dz_opt(ctx, "rays.plain_step", 0) != 0 ? 1 : 0;
    A.pts = nullptr; A.npts = nullptr; A.pcap = 0;
    if (dz_opt(ctx, "rays.keep_paths", 0) != 0) {
      // a ray advances half a cell per step: a few times (nnx + nnz) points even for a path that wanders; longer ones are flagged
      A.pcap = 4 * (g.nnx + g.nnz) + 16;
      if ((rc = dz_scratch(ctx, "rays.pts", nr1 * (size_t)A.pcap, &A.pts))) return rc;
      if ((rc = dz_scratch(ctx, "rays.npts", nr1, &A.npts))) return rc;
      DZ_HIP(hipMemsetAsync(A.npts, 0, nr1 * 4, ctx->stream));
    }
    ctx->ksec["rays.path_cap"] = A.pcap;
    ctx->ksec["rays.path_rays"] = A.pts ? (double)nray : 0.0;
    twin = dz_opt(ctx, "rays.dense_twin", 0) != 0 && !A.keep_small;
    A.dense = twin ? 2 : 0;
    A.countd = nullptr;
    if (twin) {
      if ((rc = dz_scratch(ctx, "rays.countd", (size_t)(nray + 1), &A.countd))) return rc;
      DZ_HIP(hipMemsetAsync(A.countd, 0, (size_t)(nray + 1) * 8, ctx->stream));
    }
    if ((rc = dz_scratch(ctx, "rays.nlist", nr1, &A.nlist))) return rc;
    if ((rc = dz_scratch(ctx, "rays.lcell", nr1 * A.LK, &A.lcell))) return rc;
    if ((rc = dz_scratch(ctx, "rays.lval", nr1 * A.LK * (joint ? 3 : 1), &A.lval))) return rc;
    // the caller may announce rows it is going to append (regularisation): the CSR arrays then get that much slack and
    // dazim_csr_append_coo writes behind the ray rows instead of reallocating and copying the matrix
    // By default: one regularisation row per model parameter with the 7-point stencil of inv/TikhRegul.f90 (a few MB).
    // (map mode: the 5-point stencil of dazim_csr_append_laplacian2d on every map)
    res_rows = (int64_t)g.nvx * g.nvz * (map ? kmax : nz - 1) * (joint ? 3 : 1);
    res_nnz = (map ? 5 : 7) * res_rows;
    if (dz_opt(ctx, "csr.reserve_rows", 0) > res_rows) res_rows = dz_opt(ctx, "csr.reserve_rows", 0);
    if (dz_opt(ctx, "csr.reserve_nnz", 0) > res_nnz) res_nnz = dz_opt(ctx, "csr.reserve_nnz", 0);
    if ((rc = dz_big_get(ctx, (size_t)(nray + res_rows + 1), &arrays.rp))) return rc;
    A.dsurf = d.dsurf.dev;
    A.rowptr = (const long *)arrays.rp; A.val = nullptr; A.col = nullptr;
    return 0;
  }
  // the kernel of each pass: count / emit x iso / joint x column-major / tiled fields x 3-D / map rows
  template <int I> static const void *kernel_no() { return (const void *)rays_kernel<(I & 8) != 0, (I & 4) != 0, (I & 2) != 0, (I & 1) != 0>; }
  const void *kern(bool emit) const {
    static const void *const tab[16] = {kernel_no<0>(),  kernel_no<1>(),  kernel_no<2>(),  kernel_no<3>(), kernel_no<4>(),  kernel_no<5>(),
                                        kernel_no<6>(),  kernel_no<7>(),  kernel_no<8>(),  kernel_no<9>(), kernel_no<10>(), kernel_no<11>(),
                                        kernel_no<12>(), kernel_no<13>(), kernel_no<14>(), kernel_no<15>()};
    return tab[(emit ? 8 : 0) + (joint ? 4 : 0) + (tiled ? 2 : 0) + (map ? 1 : 0)];
  }
  int launch(bool emit, const RayArgs &R, long nwg_) {
    RayArgs args = R;
    void *params[] = {&args};
    DZ_HIP(hipLaunchKernel(kern(emit), dim3((unsigned)nwg_), dim3(64), params, lds, ctx->stream));
    return 0;
  }
  int launch_shape() {
    lds = (size_t)A.lcap * 2 * RPW_MAX + 16;   // one cell list per ray of the wavefront
    DZ_HIP(hipFuncSetAttribute(kern(false), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DZ_HIP(hipFuncSetAttribute(kern(true), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = (int)(160 * 1024 / (lds + 256));
    {   // resident workgroups per CU are limited by LDS or by registers (3 wavefronts per SIMD): persistent workgroups beyond
        // that only queue up behind the resident ones and unbalance the XCD-ordered ray ranges
      int occ = 0;
      const void *kf = kern(false);
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kf, 64, lds) == hipSuccess && occ > 0 && occ < per_cu) per_cu = occ;
    }
    if (per_cu > 16) per_cu = 16;
    if (per_cu < 1) return dz_fail(ctx, DAZIM_E_BAD_ARG, "inversion grid too large for the LDS cell lists");
    if (dz_opt(ctx, "rays.wg_per_cu", 0) > 0 && dz_opt(ctx, "rays.wg_per_cu", 0) < per_cu) per_cu = dz_opt(ctx, "rays.wg_per_cu", 0);
    nwg = (long)ctx->num_cu * per_cu;
    if (nwg > (nray + RPW_MAX - 1) / RPW_MAX) nwg = (nray + RPW_MAX - 1) / RPW_MAX;
    if (dz_opt(ctx, "rays.nwg", 0) > 0 && dz_opt(ctx, "rays.nwg", 0) < nwg) nwg = dz_opt(ctx, "rays.nwg", 0);   // test knob: few slots serve many rays
    if (nwg >= 8) nwg -= nwg % 8;   // the XCD-aware ray order wants a multiple of 8
    if (nwg < 1) nwg = 1;
    // The Frechet slots must be all zeros when the first pass starts; every ray leaves its slot as it found it (rays_kernel).  The
    // block is cached by name across calls, grids and forms (a slot of this call may straddle slots of the last one, and a new block
    // holds anything), so it is cleared here, once per call, on the stream the passes run on.
    const size_t nslot = (size_t)nwg * RPW_MAX * (g.nvx + 2) * (g.nvz + 2) * (joint ? 3 : 1);
    int rc;
    if ((rc = dz_scratch(ctx, "rays.fdm", nslot, &A.fdm_scratch))) return rc;
    DZ_HIP(hipMemsetAsync(A.fdm_scratch, 0, nslot * sizeof(float), ctx->stream));
    ctx->ksec["rays.nwg"] = (double)nwg;
    return 0;
  }
  int sort_rays() {   // ... and the task counters of the passes
    int rc;
    A.perm = nullptr;
    if (nray >= 64 && nray < (1ll << 32) && dz_opt(ctx, "rays.sort", 1) != 0) {
      int fbits = 1;
      while ((1ll << fbits) < nfield) fbits++;
      const int dbits = 32 - fbits > 12 ? 12 : 32 - fbits;
      if (dbits >= 4) {
        unsigned *k0, *k1, *v0, *v1;
        if ((rc = dz_scratch(ctx, "rays.sortbuf", (size_t)nray * 4 + 16, &k0))) return rc;
        k1 = k0 + nray; v0 = k1 + nray; v1 = v0 + nray;
        const float ex = (float)g.nnx * g.dnx, ez = (float)g.nnz * g.dnz;
        const float inv_dmax = 1.0f / sqrtf(ex * ex + ez * ez);
        hipLaunchKernelGGL(k_ray_keys, dim3((unsigned)((nray + 255) / 256)), dim3(256), 0, ctx->stream, (long)nray, d.field.dev, d.scx.dev,
                           d.scz.dev, d.rcx.dev, d.rcz.dev, inv_dmax, dbits, k0, v0, overlap ? A.tslot : (const int *)nullptr);
        size_t tb = 0;
        DZ_HIP(rocprim::radix_sort_pairs(nullptr, tb, k0, k1, v0, v1, (size_t)nray, 0, fbits + dbits, ctx->stream));
        void *tmp;
        if ((rc = dz_scratch(ctx, "rays.sorttmp", tb + 256, &tmp))) return rc;
        DZ_HIP(rocprim::radix_sort_pairs(tmp, tb, k0, k1, v0, v1, (size_t)nray, 0, fbits + dbits, ctx->stream));
        A.perm = v1;
      }
    }
    if ((rc = dz_scratch(ctx, "rays.qcount", 32, &A.qcount))) return rc;
    DZ_HIP(hipMemsetAsync(A.qcount, 0, 128, ctx->stream));
    if (overlap) {
      const size_t nq = (size_t)((nray + RPW_MAX - 1) / RPW_MAX) + 8;
      if ((rc = dz_scratch(ctx, "rays.defer", nq, &A.defer_mark))) return rc;
      DZ_HIP(hipMemsetAsync(A.defer_mark, 0, nq * 4, ctx->stream));
    }
    return 0;
  }
  int count_pass() { return nray > 0 ? launch(false, A, nwg) : 0; }
  // ---- the count pass beside the eikonal launch's tail: a sequence of NON-BLOCKING passes on the third stream ----
  // A pass traces every quad of rays whose fields are finished and marks the others; the host launches the next pass a moment
  // later for the marked ones, and a last one after the eikonal call is complete (spill reruns included).  The first pass goes
  // out when the eikonal launch's task queue is nearly empty (the kernel reports the tasks it has handed out through
  // host-mapped words): from then on its workgroups leave and the passes' workgroups take their slots.  No ray workgroup ever
  // waits for the eikonal kernel, so nothing depends on which launch's wavefronts the hardware keeps resident.
  int count_passes_beside_eikonal() {
    int rc;
    const auto t_poll0 = std::chrono::steady_clock::now();
    auto fmm_over = [&]() {
      const bool over = hipEventQuery(ctx->ev_f1) == hipSuccess;
      if (!over) (void)hipGetLastError();
      return over;
    };
    if (ctx->fields.hprog && ctx->fields.total_tasks > 0) {
      const unsigned slack = ctx->fields.nwg / 4 + 8 * 16;
      const unsigned total = ctx->fields.total_tasks;
      const unsigned want = total > slack ? total - slack : 0;
      for (;;) {
        unsigned have = 0;
        for (int c = 0; c < 8; c++) have += ctx->fields.hprog[c];
        if (have >= want || fmm_over()) break;
        if (std::chrono::steady_clock::now() - t_poll0 > std::chrono::seconds(120)) break;
        usleep(50);
      }
    }
    const unsigned nquad_all = (unsigned)((nray + RPW_MAX - 1) / RPW_MAX);
    unsigned pending = nquad_all, *h_traced = nullptr;
    { void *hp; if ((rc = dz_pinned(ctx, "rays.host_pending", 64, &hp))) return rc; h_traced = (unsigned *)hp; }
    DZ_HIP(hipMemsetAsync(A.defer_mark, 1, (size_t)nquad_all * 4, ctx->stream));   // every quad marked (any non-zero value)
    int npass = 0;
    bool collected = false, ev0_set = false;
    unsigned left_by_first = 0;
    int rcf = 0;
    while (pending > 0) {
      const bool last = fmm_over();
      if (last && !collected) {   // the eikonal call's own end: statuses, spill reruns (main stream), before the pass that needs every field
        swap.restore();
        DZ_HIP(hipStreamSynchronize(ctx->stream3));   // (the preparation and the passes so far ran there: the last pass runs on the main stream)
        rcf = dz_fmm_finish(ctx);
        collected = true;
        if (rcf) break;
        if (npass == 0) (void)hipEventRecord(ctx->ev_r1, ctx->stream);   // (nothing ran beside the launch)
        (void)hipEventRecord(ctx->ev0, ctx->stream);                     // what follows the eikonal launch's end is what the step pays
        ev0_set = true;
      }
      long nwg_pass = nwg;
      A.max_quads = 0;
      A.sweeps = collected ? 1 : 3;   // (measured: 1 -> 300-302 ms, 2-4 -> 297.6-299.6, 6 -> 301-302, 12 -> 305.6, 32 -> 319.6: every look costs)
      if (collected) A.fdone = nullptr;
      DZ_HIP(hipMemsetAsync(A.qcount, 0, 32, ctx->stream));        // the count pass's task counters
      if ((rc = launch(false, A, nwg_pass))) return rc;
      if (!collected) DZ_HIP(hipEventRecord(ctx->ev_r1, ctx->stream));
      DZ_HIP(hipMemcpyAsync(h_traced, A.qcount + 18, 4, hipMemcpyDeviceToHost, ctx->stream));
      DZ_HIP(hipStreamSynchronize(ctx->stream));
      const unsigned before = pending;
      pending = collected ? 0u : nquad_all - *h_traced;
      if (npass == 0) left_by_first = pending;
      npass++;
      if (pending > 0 && pending == before) usleep(100);   // (nothing was ready: let a few more fields finish)
    }
    swap.restore();
    if (!collected) rcf = dz_fmm_finish(ctx);
    DZ_HIP(hipStreamSynchronize(ctx->stream3));
    if (rcf) return rcf;
    ctx->ksec["rays.passes"] = npass;
    ctx->ksec["rays.deferred_quads"] = left_by_first;   // quads the first pass had to leave (fields still marching, or waiting for their rerun)
    A.fdone = nullptr; A.defer_mark = nullptr; A.max_quads = 0; A.sweeps = 1;
    // what the step pays for the rays: from the end of the eikonal launch on (the passes' share beside it is free) = the last
    // pass beside the launch, as far as it outlasted it, + everything below
    float ms_tail = 0;
    if (hipEventElapsedTime(&ms_tail, ctx->ev_f1, ctx->ev_r1) == hipSuccess && ms_tail > 0) overlap_tail_s = ms_tail * 1e-3;
    if (!ev0_set) (void)hipEventRecord(ctx->ev0, ctx->stream);
    return 0;
  }
  // exclusive scan of the row counts -> M.rp, the arrays of that many entries (+ slack), the emit pass.  G, and then its dense
  // twin: a second emit pass over the saved cell lists (no ray is traced again unless its list did not fit)
  int scan_and_emit(Arrays &M, long *count, int64_t slack, bool dense_twin) {
    int rc; void *p; size_t tb = 0;
    DZ_HIP(rocprim::exclusive_scan(nullptr, tb, count, (long *)M.rp, 0l, (size_t)(nray + 1), rocprim::plus<long>(), ctx->stream));
    if ((rc = dz_scratch(ctx, "rays.scan", tb + 256, &p))) return rc;
    DZ_HIP(rocprim::exclusive_scan(p, tb, count, (long *)M.rp, 0l, (size_t)(nray + 1), rocprim::plus<long>(), ctx->stream));
    DZ_HIP(hipMemcpyAsync(&M.nnz, M.rp + nray, 8, hipMemcpyDeviceToHost, ctx->stream));
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    M.cap_nnz = M.nnz + slack;   // (options csr.reserve_rows / csr.reserve_nnz: room for rows appended later)
    const size_t cap = (size_t)(M.cap_nnz > 0 ? M.cap_nnz : 1);
    if ((rc = dz_big_get(ctx, cap, &M.v)) || (rc = dz_big_get(ctx, cap, &M.cl))) return rc;
    RayArgs R = A;
    R.rowptr = (const long *)M.rp; R.val = M.v; R.col = M.cl;
    if (dense_twin) {
      R.dense = 1;
      DZ_HIP(hipMemsetAsync(A.qcount + 8, 0, 32, ctx->stream));   // the emit pass's task counters
    }
    return nray > 0 ? launch(true, R, nwg) : 0;
  }
  int statuses() {   // first failing ray is the reference's STOP
    int rc;
    std::vector<int> hs(nr1), hb(nr1);
    unsigned hq[2] = {0, 0};
    if (nray > 0) {
      DZ_HIP(hipMemcpyAsync(hq, A.qcount + 16, 8, hipMemcpyDeviceToHost, ctx->stream));
      DZ_HIP(hipMemcpyAsync(hs.data(), A.status, nray * 4, hipMemcpyDeviceToHost, ctx->stream));
      DZ_HIP(hipMemcpyAsync(hb.data(), A.rbflag, nray * 4, hipMemcpyDeviceToHost, ctx->stream));
      DZ_HIP(hipStreamSynchronize(ctx->stream));
    }
    int nb = 0, err = 0;
    for (int64_t i = 0; i < nray; i++) {
      nb += hb[i];
      if (hs[i] && !err) err = dz_fail(ctx, hs[i], "ray %ld: receiver lies outside model", (long)i);
    }
    if (n_boundary) *n_boundary = nb;
    if (nnz_out) *nnz_out = arrays.nnz;
    ctx->ksec["rays.list_sweeps"] = hq[0];     // rays that took the full-grid sweep instead of the LDS cell list
    ctx->ksec["rays.list_retraced"] = hq[1];   // rays the emit pass traced a second time
    ctx->ksec["rays.lcap"] = A.lcap;
    if ((rc = d.dsurf.finish())) return rc;
    DZ_HIP(hipStreamSynchronize(ctx->stream));
    return err;
  }
  int adopt() {
    int rc;
    const int64_t n = (int64_t)g.nvx * g.nvz * (map ? kmax : nz - 1) * (joint ? 3 : 1);
    arrays.keep = true;   // adopted (dz_csr_adopt_cap frees them itself if it fails)
    if ((rc = dz_csr_adopt_cap(ctx, nray, n, arrays.nnz, arrays.rp, arrays.cl, arrays.v, nray + res_rows, arrays.cap_nnz, G))) return rc;
    if (twin) {
      dazim_csr *Gd = nullptr;
      arrays_d.keep = true;
      if ((rc = dz_csr_adopt_cap(ctx, nray, n, arrays_d.nnz, arrays_d.rp, arrays_d.cl, arrays_d.v, 0, 0, &Gd)) || (rc = dz_csr_set_twin(ctx, *G, Gd))) {
        dazim_csr_free(ctx, *G);
        *G = nullptr;
        return rc;
      }
    }
    return 0;
  }
  int run() {
    int rc;
    if ((rc = check()) || (rc = decide_overlap()) || (rc = stage_inputs()) || (rc = kernel_constants()) || (rc = scratch()) ||
        (rc = launch_shape()) || (rc = sort_rays()))
      return rc;
    DzTimer t(ctx, "rays");
    DZ_HIP(hipMemsetAsync(A.count, 0, (size_t)(nray + 1) * 8, ctx->stream));
    if ((rc = overlap ? count_passes_beside_eikonal() : count_pass())) return rc;
    if ((rc = scan_and_emit(arrays, A.count, res_nnz, false))) return rc;
    if (twin && ((rc = dz_big_get(ctx, (size_t)(nray + 1), &arrays_d.rp)) || (rc = scan_and_emit(arrays_d, A.countd, 0, true)))) return rc;
    t.stop();
    if (overlap) {
      ctx->ksec["rays.after_fmm_count"] = overlap_tail_s;
      ctx->ksec["rays"] += overlap_tail_s;
    }
    return (rc = statuses()) ? rc : adopt();
  }
};

}  // namespace

// = the receiver loop of CalSurfG (inv/CalSurfG.f90:1326-1364) for every ray of a batch of fields
extern "C" int dazim_rays_build_G(dazim_ctx *ctx, int nx, int ny, int nz, float goxd, float gozd, float dvxd,
                                  float dvzd, int kmax, const float *vels, int nfield, const float *scx,
                                  const float *scz, const int *period, const int *kidx, const float *veln,
                                  const float *ttn, const float *ttnr, const int *nstsr, const dazim_refbox *boxes,
                                  int64_t nray, const int *field, const float *rcx, const float *rcz,
                                  const double *svs, const double *svp, const double *srho, float *dsurf,
                                  dazim_csr **G, int64_t *nnz_out, int *n_boundary) {
  RayBuild b(ctx);
  b.nx = nx; b.ny = ny; b.nz = nz; b.goxd = goxd; b.gozd = gozd; b.dvxd = dvxd; b.dvzd = dvzd;
  b.kmax = kmax; b.vels = vels; b.svs = svs; b.svp = svp; b.srho = srho;
  b.nfield = nfield; b.scx = scx; b.scz = scz; b.period = period; b.kidx = kidx;
  b.veln = veln; b.ttn = ttn; b.ttnr = ttnr; b.nstsr = nstsr; b.boxes = boxes;
  b.nray = nray; b.field = field; b.rcx = rcx; b.rcz = rcz;
  b.dsurf = dsurf; b.G = G; b.nnz_out = nnz_out; b.n_boundary = n_boundary;
  return b.run();
}
// = the receiver loop of CalSurfGAnisoJoint (inv/CalSurfGAniso_Joint.f90:680-752): rpathsAzim and rows
// with the three column blocks dVs | Gc | Gs; lsen = Lsen_Gsc from depthkernelTI (TI kernels, an input)
extern "C" int dazim_rays_build_G_joint(dazim_ctx *ctx, int nx, int ny, int nz, float goxd, float gozd, float dvxd,
                                        float dvzd, int kmax, const float *vels, int nfield, const float *scx,
                                        const float *scz, const int *period, const int *kidx, const float *veln,
                                        const float *ttn, const float *ttnr, const int *nstsr,
                                        const dazim_refbox *boxes, int64_t nray, const int *field, const float *rcx,
                                        const float *rcz, const double *svs, const double *svp, const double *srho,
                                        const float *lsen, float *dsurf, dazim_csr **G, int64_t *nnz_out,
                                        int *n_boundary) {
  if (!lsen) return dz_fail(ctx, DAZIM_E_BAD_ARG, "joint mode needs Lsen_Gsc");
  RayBuild b(ctx);
  b.nx = nx; b.ny = ny; b.nz = nz; b.goxd = goxd; b.gozd = gozd; b.dvxd = dvxd; b.dvzd = dvzd;
  b.kmax = kmax; b.vels = vels; b.svs = svs; b.svp = svp; b.srho = srho; b.lsen = lsen;
  b.nfield = nfield; b.scx = scx; b.scz = scz; b.period = period; b.kidx = kidx;
  b.veln = veln; b.ttn = ttn; b.ttnr = ttnr; b.nstsr = nstsr; b.boxes = boxes;
  b.nray = nray; b.field = field; b.rcx = rcx; b.rcz = rcz;
  b.dsurf = dsurf; b.G = G; b.nnz_out = nnz_out; b.n_boundary = n_boundary;
  return b.run();
}

// Map rows (the per-period phase-velocity / 2-psi map inversion): the same receiver loop with the Frechet values themselves as the
// row entries -- fdm (, fdmc, fdms when azim) -- in one column block per period: what dazim_rays_build_G / _joint emit with unit
// depth kernels (sen_vs = 1, sen_vp = sen_rho = 0, Lsen_Gsc = 1) and nz = 2, bit for bit, with the period folded into the column
// blk*kmax*ncell + (period_idx-1)*ncell + (jj-1)*nvx + kk-1.  No model, no depth-kernel tables.
extern "C" int dazim_rays_build_G_maps(dazim_ctx *ctx, int nx, int ny, float goxd, float gozd, float dvxd, float dvzd, int kmax,
                                       int azim, int nfield, const float *scx, const float *scz, const int *period,
                                       const float *veln, const float *ttn, const float *ttnr, const int *nstsr,
                                       const dazim_refbox *boxes, int64_t nray, const int *field, const float *rcx,
                                       const float *rcz, float *dsurf, dazim_csr **G, int64_t *nnz_out, int *n_boundary) {
  RayBuild b(ctx);
  b.map = true; b.azim = azim != 0;
  b.nx = nx; b.ny = ny; b.nz = 2; b.goxd = goxd; b.gozd = gozd; b.dvxd = dvxd; b.dvzd = dvzd;
  b.kmax = kmax; b.nfield = nfield; b.scx = scx; b.scz = scz; b.period = period;
  b.veln = veln; b.ttn = ttn; b.ttnr = ttnr; b.nstsr = nstsr; b.boxes = boxes;
  b.nray = nray; b.field = field; b.rcx = rcx; b.rcz = rcz;
  b.dsurf = dsurf; b.G = G; b.nnz_out = nnz_out; b.n_boundary = n_boundary;
  return b.run();
}

// The ray geometries of the last dazim_rays_build_G[_joint] call made with option "rays.keep_paths" = 1: what the reference
// writes to raypath_refmdl_<T>s.dat when writepath is set (fwd/rpathsAzim.f90:617-625, fwd/FwdTraveltimeCPS.f90:673-691).
// dims: *nray rays, *cap points per ray at most.  copy: xz[nray][cap][2] (colatitude, longitude in rad) and nrp[nray]
// (number of points, receiver first, source last; -1: more than cap points) into host or device arrays.
extern "C" int dazim_ray_paths_dims(dazim_ctx *ctx, int64_t *nray, int *cap) {
  if (!ctx || !nray || !cap) return DAZIM_E_BAD_ARG;
  *nray = (int64_t)dazim_last_kernel_seconds(ctx, "rays.path_rays");
  *cap = (int)dazim_last_kernel_seconds(ctx, "rays.path_cap");
  if (*nray < 0) *nray = 0;
  if (*cap < 0) *cap = 0;
  return 0;
}
extern "C" int dazim_ray_paths_copy(dazim_ctx *ctx, float *xz, int *nrp) {
  int64_t nray;
  int cap;
  if (!ctx || !xz || !nrp || dazim_ray_paths_dims(ctx, &nray, &cap)) return DAZIM_E_BAD_ARG;
  if (nray == 0 || cap == 0) return dz_fail(ctx, DAZIM_E_BAD_ARG, "no ray paths were kept (option rays.keep_paths)");
  auto a = ctx->scratch.find("rays.pts"), b = ctx->scratch.find("rays.npts");
  if (a == ctx->scratch.end() || b == ctx->scratch.end()) return dz_fail(ctx, DAZIM_E_BAD_ARG, "no ray paths were kept");
  DZ_HIP(hipMemcpyAsync(xz, a->second.first, (size_t)nray * cap * 8, hipMemcpyDefault, ctx->stream));
  DZ_HIP(hipMemcpyAsync(nrp, b->second.first, (size_t)nray * 4, hipMemcpyDefault, ctx->stream));
  DZ_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}
