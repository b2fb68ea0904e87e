/* dazim.h -- C ABI of the MI355X-native DAzimSurfTomo hot path (libdazim_hip.so).
 *
 * The reference (Chuanming-Liu/DAzimSurfTomo) has no FFI; its seams are Fortran procedure calls
 * with module-global state.  Each entry point below replaces one seam and
 * cites it as inv/<file>:<line> (inv/ = src/src_inv_iso_joint/).  The Fortran host binds them
 * through ISO_C_BINDING (host/dazim_mod.f90).
 *
 * Conventions
 *  - every function returns 0 on success, >0 for a reference-STOP-equivalent condition
 *    (DAZIM_E_*), <0 for a HIP/RCCL runtime failure; dazim_last_error(ctx) holds the message.
 *  - every bulk pointer may be a HOST pointer or a DEVICE (hipMalloc) pointer; the library
 *    detects which.  Host pointers are staged through device buffers (PCIe-inclusive); device
 *    pointers are used in place (zero-copy, what bench.py times).
 *  - 2-D grids keep the reference's Fortran memory order: node (iz,ix) of an nnz x nnx grid is at
 *    [(ix-1)*nnz + (iz-1)], i.e. "[ix][iz]" in C terms.  Model cubes are vel(nx,ny,nz) =
 *    [k][j][i] in C terms.  Indices that cross the ABI (period_idx, COO/CSR columns) are 1-based
 *    exactly where the reference's are, and say so.
 *  - no global state: everything hangs off dazim_ctx; one ctx per GPU / per host thread.
 */
#ifndef DAZIM_H
#define DAZIM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAZIM_RMAX 129 /* refined source grid is at most (2*sgs*sgdl+1)^2, inv/CalSurfG.f90:1187-1196 */

enum {
  DAZIM_OK = 0,
  DAZIM_E_SOURCE_OUTSIDE = 1,   /* inv/CalSurfG.f90:287-293, 1174-1180 */
  DAZIM_E_RECEIVER_OUTSIDE = 2, /* inv/CalSurfG.f90:1649-1655, 1863-1869 */
  DAZIM_E_NNZ_OVERFLOW = 4,     /* inv/Main_Jt.f90:523 "increase sparsity fraction" */
  DAZIM_E_BAD_ARG = 5,
  DAZIM_E_ROOT_NOT_FOUND = 6    /* inv/surfdisp96.f:307-348 (warning there; count returned here) */
};

typedef struct dazim_ctx dazim_ctx;

/* propagation-grid geometry derived from the inversion grid, inv/CalSurfG.f90:1017-1038 */
typedef struct {
  int nvx, nvz;             /* B-spline vertices nx-2, ny-2                      */
  int nnx, nnz;             /* propagation nodes (nvx-1)*5+1, (nvz-1)*5+1         */
  float gox, goz, dnx, dnz; /* origin (colatitude, longitude; rad) and node step  */
  float dvx, dvz;           /* vertex step (rad)                                  */
} dazim_geom;

/* refined source box of one field, inv/CalSurfG.f90:1187-1206,1266-1271 */
typedef struct {
  int vnl, vnr, vnt, vnb; /* box bounds in coarse node indices, 1-based */
  int nnxr, nnzr;         /* refined grid size                           */
  int isx, isz;           /* coarse source cell                          */
  float goxr, gozr, dnxr, dnzr;
} dazim_refbox;

/* ---- context / memory ---------------------------------------------------------------------- */
int dazim_create(dazim_ctx **ctx, int device);
void dazim_destroy(dazim_ctx *ctx);
const char *dazim_last_error(const dazim_ctx *ctx);
int dazim_malloc(dazim_ctx *ctx, void **dptr, size_t bytes);
int dazim_free(dazim_ctx *ctx, void *dptr);
/* blocking copies on the context's stream.  After an asynchronous dazim_dispersion_kernels call (option disp.async) a copy that
 * touches the model or one of the three kernel tables waits for the perturbed copies on the auxiliary stream first; any other
 * copy leaves them running (dazim_get_stat "aux.pending") */
int dazim_memcpy_h2d(dazim_ctx *ctx, void *dst, const void *src, size_t bytes);
int dazim_memcpy_d2h(dazim_ctx *ctx, void *dst, const void *src, size_t bytes);
int dazim_sync(dazim_ctx *ctx);
/* 64-bit hash of every byte of a host array (host/dazim_mod.f90's aprod keys its cached device matrix on iw and rw with it,
 * replaces nothing in the reference: inv/aprod.f90:7 reads the arrays afresh on every call, which this makes observable) */
unsigned long long dazim_hash64(const void *data, size_t bytes);
void *dazim_stream(dazim_ctx *ctx); /* the hipStream_t every kernel of this ctx is launched on */
/* seconds spent in the last call's kernels, measured with HIP events on the ctx stream; name
 * selects the kernel ("fmm", "gridder", "disp", "ti", "rays", "spmv", "spmvt", "lsmr", "vs_kernels", "column_lsq"); <0 if unknown */
double dazim_last_kernel_seconds(const dazim_ctx *ctx, const char *name);
/* the same table with a status: times of the last call's kernels AND the counts / choices the library reports ("fmm.wg_per_cu",
 * "spmv.kind", "lsmr.nranks", "fmm.field_pops" ...; docs/OPTIONS.md).  0 and *value, or DAZIM_E_BAD_ARG for an unknown name.      */
int dazim_get_stat(const dazim_ctx *ctx, const char *name, double *value);
/* tuning / test knobs, none of which changes a result unless its entry says so: the catalogue is docs/OPTIONS.md (heap forms and
 * time slicing of the eikonal kernel "fmm.*", two-stream dispersion "disp.*", ray cell lists "rays.*", product kernels "spmv.*",
 * "lsmr.*", CSR reservations "csr.*").  The environment variable DAZIM_OPTS=name=value,... sets options when a context is made. */
int dazim_set_option(dazim_ctx *ctx, const char *name, int value);

/* ---- geometry (host only; replaces the constant block inv/CalSurfG.f90:1005-1038) ---------- */
int dazim_geometry(int nx, int ny, float goxd, float gozd, float dvxd, float dvzd, dazim_geom *g);

/* ---- K1: dispersion + depth kernels -------------------------------------------------------------
 * = depthkernel (inv/CalSurfG.f90:1-139): per model column Brocher Vp(Vs), rho(Vp), knot -> layer
 *   refinement (refineGrid2LayerMdl, :2317), surfdisp96 (inv/surfdisp96.f:52; iflsph=1, Rayleigh,
 *   fundamental mode, phase velocity) for the column and its 6*nz perturbed copies, central
 *   differences.  With sen_* == NULL only pvRc is produced (= CalRayleighPhase,
 *   fwd/FwdTraveltimeCPS.f90:4).
 *  vel   [nz][ny][nx] fp32 (= Fortran vel(nx,ny,nz));  depz [nz] (host);  periods [kmax] (host)
 *  pvRc  [kmax][nx*ny] fp64 holding fp32-rounded values (cg(k)=sngl(c(k)), inv/surfdisp96.f:292)
 *  sen_vs, sen_vp, sen_rho [nz][kmax][nx*ny] fp64, nullable (all three or none)
 *  n_failed  number of (column, period) entries for which no root was found (pvRc = 0 there,
 *            inv/surfdisp96.f:342-348); the reference only prints a warning                    */
int dazim_dispersion_kernels(dazim_ctx *ctx, int nx, int ny, int nz, const float *vel,
                             const float *depz, float sublayers, int kmax, const double *periods,
                             double *pvRc, double *sen_vs, double *sen_vp, double *sen_rho,
                             int *n_failed);

/* ---- surfdisp96 itself, every argument -------------------------------------------------------------
 * = surfdisp96(thkm,vpm,vsm,rhom,nlayer,iflsph,iwave,mode,igr,kmax,t,cg) (inv/surfdisp96.f:52-354) for a batch of
 *   layered models: iflsph 0 flat / 1 spherical (sphere, :480); iwave 1 Love (dltar1, :704) / 2 Rayleigh (dltar4,
 *   :767, with the water-layer branch :844 when vs of the first layer is <= 0); mode 1 = fundamental, 2 = first
 *   higher, ... (:217); igr 0 phase velocity / > 0 group velocity from the roots at T/(1+h), T/(1-h), h = 0.005
 *   (:226-233, :276-304).  dazim_dispersion_kernels above is the tuned form of the one combination the reference's
 *   programs call (1, 2, 1, 0); this entry is the subroutine as it stands, one lane per model.
 *  nlayer [nmodel] layers of each model (<= nlayer_max <= 200 = NL); thk, vp, vs, rho [nmodel][nlayer_max] fp32
 *  (thickness of the last layer = half-space, ignored); periods [kmax <= 60 = NP] fp64 (host)
 *  cg [nmodel][kmax] fp64 holding fp32-rounded values, 0 from the first period without a root on (:342-348)
 *  n_failed  number of (model, period) entries left at 0, nullable                                        */
int dazim_surfdisp96(dazim_ctx *ctx, int nmodel, int nlayer_max, const int *nlayer, const float *thk, const float *vp,
                     const float *vs, const float *rho, int iflsph, int iwave, int mode, int igr, int kmax,
                     const double *periods, double *cg, int *n_failed);

/* ---- K1 for every wave type: dispersion + depth kernels of Rayleigh / Love, phase / group velocities in one table -----------
 * = depthkernel (inv/CalSurfG.f90:1-139) called once per segment with that segment's (iwave, igr): mode 1, iflsph 1, the same
 *   Brocher / refineGrid2LayerMdl / +-0.5 % arithmetic as dazim_dispersion_kernels.  The tables are indexed by a "virtual period":
 *   the segments' periods laid end to end, K = sum of seg_kmax, which is all that dazim_fmm_batch, dazim_rays_build_G*,
 *   dazim_vs_kernels and the column solves see of a wave type.
 *  nseg 1..4; seg_iwave [nseg] 1 Love / 2 Rayleigh; seg_igr [nseg] 0 phase / 1 group; seg_kmax [nseg] 1..60 (host arrays); a pair
 *  (iwave, igr) may appear once.  periods [K] (host), segment after segment.  vel, depz, sublayers as for dazim_dispersion_kernels.
 *  pv [K][nx*ny]; sen_vs, sen_vp, sen_rho [nz][K][nx*ny] fp64, nullable (all three or none; one or two of them: refused)
 *  The Rayleigh-phase segment (2, 0) is computed by dazim_dispersion_kernels and its rows are that call's bits; a call whose only
 *  segment it is IS that call.  The other segments run surfdisp96's own root search (the device functions of dazim_surfdisp96) on
 *  layer stacks built on the device, one lane per (column, variant): equal, bit for bit, to depthkernel composed of
 *  dazim_surfdisp96 calls.  sen_vp of a Love segment is 0.  A curve ends at its first period without a root (pv = 0 from there on,
 *  as the subroutine leaves it; sen_* = 0 at those entries); n_failed counts such entries of all segments, nullable.
 *  With a communicator attached every rank computes every segment in full.                                            */
int dazim_dispersion_kernels_typed(dazim_ctx *ctx, int nx, int ny, int nz, const float *vel, const float *depz, float sublayers,
                                   int nseg, const int *seg_iwave, const int *seg_igr, const int *seg_kmax, const double *periods,
                                   double *pv, double *sen_vs, double *sen_vp, double *sen_rho, int *n_failed);

/* ---- N1: TI eigenfunction partials -> azimuthal depth kernels ---------------------------------------
 * = depthkernelTI (inv/depthkernelTI.f90:2) calling tregn96 (inv/tregn96.f:52) once per column: Rayleigh fundamental-mode
 *   eigenfunctions of the flattened TI column (A=C=rho*Vp^2, L=N=rho*Vs^2, F=A-2L), partials dc/dah, dc/dbv, dc/dn with the
 *   causal-Q shift (Qp=150, Qs=50) and sprayl's sphericity factors, combined over the sub-layers of each inversion layer into
 *   Lsen_Gsc = dc/dA*A + dc/dL*L, the sensitivity of c to Gc/L, Gs/L.  Solid layers only (the reference's models are).
 *  vel, depz, sublayers, periods as for dazim_dispersion_kernels; pvRc [kmax][nx*ny] = its output (the reference recomputes
 *  the same surfdisp96 curve inside depthkernelTI); Lsen_Gsc out [nz-1][kmax][nx*ny] fp32 = Fortran Lsen_Gsc(nx*ny,kmax,nz-1),
 *  0 where pvRc is 0.                                                                                             */
int dazim_ti_kernels(dazim_ctx *ctx, int nx, int ny, int nz, const float *vel, const float *depz,
                     float sublayers, int kmax, const double *periods, const double *pvRc, float *Lsen_Gsc);

/* ---- K2+K3: batched eikonal fields -----------------------------------------------------------
 * = gridder (inv/CalSurfG.f90:1423) once per period + per (source,period): bsplrefine (:1525),
 *   travel on the refined box (:258, urg=1), injection + band completion (:1246-1308) and
 *   travel on the coarse grid (urg=2), i.e. the body of the source loop inv/CalSurfG.f90:1146-1314.
 *  pv         [kmax][(nvz+2)*(nvx+2)] phase velocity per period and inversion cell (= pvRc(:,k))
 *  period_idx [nfield] 1-based period of each field (= periods(srcnum,knumi))
 *  scx, scz   [nfield] source colatitude / longitude in radians (fp32, as the reference holds them)
 *  veln       [kmax][nnx][nnz]  out, nullable: gridded velocity per period
 *  ttn        [nfield][nnx][nnz] out: coarse traveltime field
 *  ttnr       [nfield][129][129] out, nullable: refined field (0 where the node is not alive/close)
 *  nstsr      [nfield][129][129] out, nullable: refined node status (-1 far, 0 alive, >0 close,
 *             -9 outside the nnzr x nnxr box)
 *  boxes      [nfield] out, nullable
 *  status     [nfield] out, nullable: DAZIM_OK or DAZIM_E_SOURCE_OUTSIDE per field; the call
 *             returns the first non-zero status (the reference STOPs there)                    */
/* ttn nullable (round 6): the coarse fields then stay inside the library, in the eikonal kernel's own layout, for the
 * dazim_rays_build_G* call that follows with ttn = NULL -- the reference's CalSurfG returns no field either (inv/CalSurfG.f90:909-912).
 * With option "fmm.async" = 1 on top (and every array device-resident) the call returns when its launch is enqueued; the ray call
 * that follows runs beside the launch's tail and collects this call's statuses and errors (docs/OPTIONS.md).                     */
int dazim_fmm_batch(dazim_ctx *ctx, int nx, int ny, float goxd, float gozd, float dvxd, float dvzd,
                    int kmax, const double *pv, int nfield, const float *scx, const float *scz,
                    const int *period_idx, float *veln, float *ttn, float *ttnr, int *nstsr,
                    dazim_refbox *boxes, int *status);

/* ---- K6/K7: sparse matrix + LSMR ----------------------------------------------------------------
 * The reference stores G as COO triplets rw / iw(2:nar+1) rows / iw(nar+2:2nar+1) cols
 * (inv/aprod.f90:20-24).  dazim_csr keeps the same matrix on the device twice: CSR for A*x and the
 * stable transpose (CSC) for A^T*y, fp32 values + int32 indices, int64 pointers.               */
typedef struct dazim_csr dazim_csr;

/* build from the reference's COO arrays (1-based irow/icol, rows need not be sorted).  nnz order
 * inside a row is kept, so sums run over the row in the order the reference appended it.        */
int dazim_csr_from_coo(dazim_ctx *ctx, int64_t m, int64_t n, int64_t nnz, const int *irow,
                       const int *icol, const float *rw, dazim_csr **A);
int dazim_csr_free(dazim_ctx *ctx, dazim_csr *A);
int dazim_csr_dims(const dazim_csr *A, int64_t *m, int64_t *n, int64_t *nnz);
/* multiply every stored entry of row i by w[i] (rw(i)=rw(i)*datweight(iw(1+i)), inv/Main_Jt.f90:467) */
int dazim_csr_scale_rows(dazim_ctx *ctx, dazim_csr *A, const float *w);

/* out[n] = column sums of |A|: the reference's DWS (norm(col(i))+=abs(rw(i)), inv/Main_Jt.f90:477-481) */
int dazim_csr_col_abs_sums(dazim_ctx *ctx, const dazim_csr *A, float *out);

/* device arrays in, ownership taken: rowptr[m+1] int64, col[nnz] 0-based int32, val[nnz] fp32   */
int dazim_csr_adopt(dazim_ctx *ctx, int64_t m, int64_t n, int64_t nnz, int64_t *rowptr, int *col,
                    float *val, dazim_csr **A);
/* append rows m+1..m+extra_m given as COO with absolute 1-based row ids: how the reference adds its
 * Tikhonov rows to the same triplet arrays (inv/TikhRegul.f90:2, inv/Main_Jt.f90:513-532)       */
int dazim_csr_append_coo(dazim_ctx *ctx, dazim_csr *A, int64_t extra_m, int64_t nnz, const int *irow,
                         const int *icol, const float *rw);
/* the matrix back as the reference's triplets (1-based, rows ascending); any pointer may be NULL  */
int dazim_csr_to_coo(dazim_ctx *ctx, const dazim_csr *A, int *irow, int *icol, float *rw);
/* Ray geometries (the reference's raypath_refmdl_<T>s.dat, written when `writepath` is set: fwd/rpathsAzim.f90:617-625,
 * fwd/FwdTraveltimeCPS.f90:673-691).  With option "rays.keep_paths" = 1 dazim_rays_build_G[_joint] keeps the points rgx/rgz(1:nrp)
 * of every ray -- receiver first, one point per half-cell step (after the clipping to the grid), source last -- on the device.
 * dazim_ray_paths_dims: rays and the capacity in points per ray of the last such call; dazim_ray_paths_copy: xz[nray][cap][2]
 * (colatitude, longitude in rad) and nrp[nray] (points of each ray; -1 if it needed more than cap) into host or device arrays. */
int dazim_ray_paths_dims(dazim_ctx *ctx, int64_t *nray, int *cap);
int dazim_ray_paths_copy(dazim_ctx *ctx, float *xz, int *nrp);
/* The reference keeps every ray row twice: the triplets rw/iw/col with |row| > ftol, which LSMR sees (inv/CalSurfG.f90:1358), and
 * the dense GVs (GGc, GGs) its residual diagnostics multiply with (inv/CalSigamNorm.f90:73): every entry of the cells with
 * |fdm| >= ftol, the dVs block formed with the Brocher derivatives coe_a / coe_rho left over from the LAST such cell of the ray
 * (the second loop, inv/CalSurfG.f90:1369-1378 / inv/CalSurfGAniso_Joint.f90:759-775, does not recompute them).  With option
 * "rays.dense_twin" = 1 dazim_rays_build_G[_joint] builds that second matrix as well (one more pass over the saved cell lists,
 * no second ray trace) and attaches it to G; this call hands it out (NULL if G has none).  The caller frees it. */
int dazim_csr_take_twin(dazim_ctx *ctx, dazim_csr *G, dazim_csr **twin);
/* B = the entries of A with |value| > tol (same shape, same order): the second threshold of the row assembly
 * (inv/CalSurfG.f90:1358) applied to a matrix that was built with option "rays.keep_small" = 1 (every non-zero entry of the
 * |fdm| >= ftol cells, the forward program's GGc/GGs, fwd/FwdTraveltimeCPS.f90:694-712) -- two streaming passes on the device.
 * reserve_rows / reserve_nnz: room for regularisation rows appended to B in place. */
int dazim_csr_threshold(dazim_ctx *ctx, const dazim_csr *A, float tol, int64_t reserve_rows, int64_t reserve_nnz,
                        dazim_csr **B);

/* ---- K4+K5: receiver times, ray tracing, Frechet weights, G rows ---------------------------------
 * = the receiver loop of CalSurfG (inv/CalSurfG.f90:1326-1364): srtimes (:1599), rpaths (:1735) and
 *   the row assembly with the double ftol=1e-4 threshold, for every ray of a batch whose eikonal
 *   fields (outputs of dazim_fmm_batch) are resident.  Row i of G belongs to ray i (the caller orders
 *   rays period -> source -> receiver like the reference's count1); columns are the reference's
 *   (k-1)*nvx*nvz+(jj-1)*nvx+kk, stored 0-based.
 *  vels [nz][ny][nx]; scx,scz,period_idx[nfield] as for dazim_fmm_batch; kernel_idx[nfield] 1-based
 *  period slot of sen_* (the reference's knumi; NULL = period_idx); veln,ttn,ttnr,nstsr,boxes: outputs
 *  of dazim_fmm_batch; field_of_ray[nray] 0-based; rcx,rcz[nray] receiver colatitude/longitude (rad);
 *  sen_vs,sen_vp,sen_rho [nz][kmax][nx*ny] from dazim_dispersion_kernels;
 *  tpred[nray] out = dsurf; G out; n_boundary out = rays clipped at the model edge (rbint)       */
int dazim_rays_build_G(dazim_ctx *ctx, int nx, int ny, int nz, float goxd, float gozd, float dvxd,
                       float dvzd, int kmax, const float *vels, int nfield, const float *scx,
                       const float *scz, const int *period_idx, const int *kernel_idx,
                       const float *veln, const float *ttn, const float *ttnr, const int *nstsr,
                       const dazim_refbox *boxes, int64_t nray, const int *field_of_ray,
                       const float *rcx, const float *rcz, const double *sen_vs, const double *sen_vp,
                       const double *sen_rho, float *tpred, dazim_csr **G, int64_t *nnz,
                       int *n_boundary);

/* joint Vsv + 2-psi mode: = the receiver loop of CalSurfGAnisoJoint (inv/CalSurfGAniso_Joint.f90:680-752):
 * rpathsAzim (inv/rpathsAzim.f90:16: the same ray plus per-step azimuth psi from azdist :687 and
 * cos/sin(2 psi)-weighted Frechet grids) and rows with three column blocks dVs | Gc | Gs, so
 * n = 3*(nx-2)*(ny-2)*(nz-1).  Lsen_Gsc [nz-1][kmax][nx*ny] fp32 (= Fortran Lsen_Gsc(nx*ny,kmax,nz-1))
 * are the TI depth kernels of depthkernelTI/tregn96 (inv/depthkernelTI.f90:2), an INPUT here
 * (SURVEY 8f N1).  Other arguments as dazim_rays_build_G.                                        */
int dazim_rays_build_G_joint(dazim_ctx *ctx, int nx, int ny, int nz, float goxd, float gozd, float dvxd,
                             float dvzd, int kmax, const float *vels, int nfield, const float *scx,
                             const float *scz, const int *period_idx, const int *kernel_idx,
                             const float *veln, const float *ttn, const float *ttnr, const int *nstsr,
                             const dazim_refbox *boxes, int64_t nray, const int *field_of_ray,
                             const float *rcx, const float *rcz, const double *sen_vs,
                             const double *sen_vp, const double *sen_rho, const float *Lsen_Gsc,
                             float *tpred, dazim_csr **G, int64_t *nnz, int *n_boundary);

/* ---- per-period phase-velocity and 2-psi anisotropy maps (the map inversion) --------------------------
 * The reference inverts Rayleigh phase times for the 3-D model only; the maps are the same rows BEFORE the multiplication by the
 * depth kernels (inv/CalSurfG.f90:1339-1364, inv/CalSurfGAniso_Joint.f90:728-738): dt = fdm.dc + fdmc.a1 + fdms.a2 per ray, where
 * a1 = sum_k Lsen.Gc and a2 = sum_k Lsen.Gs are the a1_cos / a2_sin columns of period_Azm_tomo.inv.
 * dazim_rays_build_G_maps: the receiver loop of CalSurfG / CalSurfGAnisoJoint (srtimes, rpaths / rpathsAzim) with the Frechet
 *   values themselves as row entries -- fdm, and fdmc, fdms when azim -- under the same double ftol rule (option rays.keep_small
 *   as there), in one column block per period: column blk*kmax*ncell + (period_idx-1)*ncell + (jj-1)*nvx + kk-1 (0-based, ncell =
 *   (nx-2)(ny-2), blk 0 c, 1 a1, 2 a2), n = kmax*ncell (x3 when azim).  Bit-identical to dazim_rays_build_G / _joint with unit depth
 *   kernels (sen_vs = 1, sen_vp = sen_rho = 0, Lsen_Gsc = 1) and nz = 2, the period folded into the column.  No model, no depth
 *   kernels; other arguments as dazim_rays_build_G (ttn = NULL and option fmm.async as there).  Option rays.dense_twin is refused
 *   (DAZIM_E_BAD_ARG).  Stat "rays.map" = 1 after such a call.
 * dazim_csr_append_laplacian2d: the 2-D analogue of dazim_csr_append_tikhonov (inv/TikhRegul.f90:2-104): nmap*ncell rows, map b
 *   regularising columns b*ncell .. with weight w[b] (host): 2w on a cell at an edge of the map, the 5-point Laplacian 4w, -w x 4
 *   inside; rows in map, j, i order; appended in place when the matrix has reserved room (csr.reserve_*, dazim_csr_threshold).
 * dazim_phase_map_update: dazim_model_update (inv/Main_Jt.f90:582-620) on the map layout: dm [kmax*ncell, x3 when azim] in/out
 *   (c block clamped to +-0.5, zeroed below 1e-5); pv [kmax][ny][nx] fp64 in/out (the dazim_fmm_batch maps): inner vertex
 *   jj*nx+kk of each period += dc in fp32, clamped to [minc, maxc], the boundary ring kept; a1, a2 [kmax][ny-2][nx-2] out (azim,
 *   nullable) = the a1 / a2 blocks (absolute values, as Gc / Gs of the joint update).  stats (host, nullable): [nblock][kmax][3] =
 *   min, max, sum |.| of the update per block and period.                                                                   */
int dazim_rays_build_G_maps(dazim_ctx *ctx, int nx, int ny, float goxd, float gozd, float dvxd, float dvzd, int kmax, int azim,
                            int nfield, const float *scx, const float *scz, const int *period_idx, const float *veln,
                            const float *ttn, const float *ttnr, const int *nstsr, const dazim_refbox *boxes, int64_t nray,
                            const int *field_of_ray, const float *rcx, const float *rcz, float *tpred, dazim_csr **G,
                            int64_t *nnz, int *n_boundary);
int dazim_csr_append_laplacian2d(dazim_ctx *ctx, dazim_csr *A, int nx, int ny, int nmap, const float *w);
int dazim_phase_map_update(dazim_ctx *ctx, int nx, int ny, int kmax, int azim, double *pv, float *dm, float minc, float maxc,
                           float *a1, float *a2, float *stats);

/* dazim_map_posterior: how well the maps are known, per period, block (c, a1, a2) and inner cell, from the matrix dazim_lsmr is given.
 *   A: the first m_data rows are the weighted data rows (unit variance after dazim_weight_data), the rows after them regularisation
 *   rows of any sparse form; columns in the map layout blk*kmax*ncell + p*ncell + cell, n = nblk*kmax*ncell (nblk = 3 with azim, else
 *   1); inside a row the columns ascend strictly (the canonical form of every dazim_csr without repeated triplets).  damp as given to
 *   dazim_lsmr.  A row touches one period only, so the normal matrix is block diagonal; per period p, with the local index
 *   a = blk*ncell + cell, n_g = nblk*ncell:
 *     D = sum_{data rows} r^T r       P = sum_{regularisation rows} l^T l + damp^2 I       A_g = D + P = R R^T       M = R^-1
 *     C = A_g^-1 = M^T M              Rm = C D = I - C P        (the resolution matrix of the regularised solve)
 *   std_post, std_noise, rdiag, rsum, width, leak: [nblk][kmax][ny-2][nx-2] fp32, the layout of dm (host or device):
 *     std_post  = sqrt(C_aa)           the posterior std, the regulariser read as a Gaussian prior of precision P
 *     std_noise = sqrt((Rm C)_aa)      unit data errors carried through the estimator alone, <= std_post
 *     rdiag     = Rm_aa                rsum = sum_c Rm_ac
 *     width     (nullable) = sqrt(sum_c Rm_ac^2 ((i_c - i_a)^2 + (j_c - j_a)^2) / sum_c Rm_ac^2) over the unknown's own block, in cells
 *               (cell = j*(nx-2) + i); 0 if the denominator is 0
 *     leak      (nullable; NULL when azim = 0) = sum_{c in the other two blocks} Rm_ac^2 / sum_{all c} Rm_ac^2: the share of the
 *               unknown's averaging kernel that lies in other kinds of unknown (the c <-> 2-psi trade-off); 0 if the denominator is 0
 *   trace [nblk][kmax] (nullable) = sum_a Rm_aa per block and period.
 *   rows [kmax][nsel][n_g] (nullable) = row sel[s] of Rm for every period (point-spread functions); sel [nsel] local indices.
 *   Arithmetic, fp64 throughout, every sum in a fixed order, no floating-point atomics, each value rounded to fp32 once:
 *     A_g(a,c) = sum over the period's rows in ascending row order of r_a r_c, then damp^2 on the diagonal;
 *     blocked right-looking Cholesky in place (panel width stat "map_post.nb"): an element's subtractions in ascending column order;
 *     M by block columns from the last: M21 = -(M22 R21) M11, the inner sums in ascending index;
 *     C_ac = sum_{i >= max(a, c)} M_ia M_ic in ascending i (the order of dazim_column_resolution);
 *     Rm_a. = e_a, then for every regularisation row l in ascending order t = sum_e C_ae l_e (ascending e), Rm_ac -= t l_c, then
 *     Rm_ac -= damp^2 C_ac; (Rm C)_aa = sum_c Rm_ac C_ac; a sum along a row: 256 strided partial sums, combined in a fixed tree.
 *   Option map_post.mfma: 1 (the default) forms the Cholesky trailing update and C with v_mfma_f64_16x16x4_f64, 0 with plain tiles.
 *   Host and device arguments give the same bits, and so do two calls.  A period whose factorisation meets a pivot that is not
 *   finite and > 0 (no regulariser and a cell without rays, non-finite entries) gets NaN in every output and is counted in n_failed
 *   (host, nullable); the other periods are unaffected.  Refused (DAZIM_E_BAD_ARG, nothing written): m_data outside 0..m, n not
 *   nblk*kmax*ncell, a missing std_post, std_noise, rdiag or rsum, leak with azim = 0, sel entries outside 0..n_g-1, rows without
 *   sel, a negative or non-finite damp, a row whose columns lie in two periods or do not ascend strictly (found on the device), n_g
 *   beyond what the row pass holds in LDS (about 16 000).  Workspace: two n_g x n_g fp64 matrices from the context's scratch, taken
 *   before the first launch.  Stats: "map_posterior" and its parts "map_post.gram", ".factor", ".inverse", ".c", ".rows" (seconds). */
int dazim_map_posterior(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, int nx, int ny, int kmax, int azim, float damp,
                        float *std_post, float *std_noise, float *rdiag, float *rsum, float *width, float *leak, int nsel,
                        const int *sel, float *rows, float *trace, int *n_failed);

/* dazim_map_tradeoff: the maps' linearised step solved exactly at K regularisation strengths, per period, with what an L-curve,
 * generalised cross-validation and the Bayesian evidence need at each.  A, m_data, nx, ny, kmax, azim, the
 * column layout and nblk are dazim_map_posterior's: a row touches one period only and its columns ascend strictly.  Every
 * regularisation row lies in one block (c, a1 or a2).  b [m_data] (host or device) is the weighted right-hand side of the data rows,
 * as dazim_lsmr is given it; the regularisation rows have right-hand side 0.
 *   scale [K][nblk], damp [K] (host): point k multiplies the stored regularisation rows of block blk by scale[k][blk], in every
 *   period, and damps with damp[k].  Per period p and point k, with the local index a = blk*ncell + cell and m_p data rows in p:
 *     D_p = sum_{data rows of p} r^T r    R_pb = sum_{regularisation rows of p in block b} l^T l    g_p = sum_{data rows of p} r^T b_r
 *     P = sum_b scale[k][b]^2 R_pb + damp[k]^2 I        A = D_p + P = R R^T        x = A^-1 g_p (forward and back substitution)
 *   Outputs (host or device; [K][kmax] unless noted):
 *     mdata_p [kmax] (nullable)  m_p
 *     chi2      |G_p x - b_p|^2 over the period's data rows     reg2 [K][kmax][nblk]  |L_pb x|^2, the rows as stored (unscaled)
 *     xnorm2    |x|^2                                            logdet_a              2 sum_i log R_ii
 *     logdet_p  (nullable; want_evidence) the same from a second factorisation, of P alone; NaN when P has a pivot that is not
 *               finite and > 0, which does not count as a failure
 *     dof [K][kmax][nblk] (nullable; want_dof)  sum_{a in block b} sum_c C_ac D_ac, C = A^-1: block b's share of tr(Rm)
 *     gcv       (nullable; want_dof)      m_p chi2 / (m_p - sum_b dof[b])^2
 *     logev     (nullable; want_evidence) -(chi2 + J)/2 + logdet_p/2 - logdet_a/2 - m_p log(2 pi)/2, J = sum_b scale[k][b]^2 reg2[b]
 *               + damp[k]^2 xnorm2
 *     x [K][n] fp32 (nullable)            the layout of dm, each value rounded once
 *   A (point, period) whose A meets a pivot that is not finite and > 0 has NaN in every output and n_failed[k][p] (host, [K][kmax],
 *   nullable) = 1, else 0; no other point and no other period is affected.  A period without data rows follows the formulas: x = 0,
 *   chi2 = 0, dof = 0.
 *   Arithmetic: fp64, every sum in a fixed order set by the problem alone, no floating-point atomics.  D_p is formed once per period
 *   and call, by dazim_map_posterior's Gram kernel on the period's data rows; a point's work matrix is D_p's row, then the period's
 *   regularisation rows in ascending row order, each product times the squared scale of the row's block, then damp^2 on the diagonal:
 *   at scale 1 and dazim_map_posterior's damp, its numbers added in its order.  The factorisation, and with want_dof the inverse and
 *   C, are its kernels (option map_post.mfma); the substitutions and fixed-order sums are dazim_model_tradeoff's.  Two calls give the
 *   same bits, host and device arguments give the same bits, and a point gives the same bits alone as at any position of any sweep.
 *   Refused (DAZIM_E_BAD_ARG, nothing written): what dazim_map_posterior refuses of A, m_data, nx, ny, kmax and n; K < 1; a missing b,
 *   scale, damp, chi2, reg2, xnorm2 or logdet_a; a negative or non-finite scale or damp; dof or gcv without want_dof; logdet_p or
 *   logev without want_evidence; a row in two periods or with columns that do not ascend strictly, a regularisation row in two
 *   blocks (found on the device); and a workspace the card's free memory cannot hold (the message names the GiB needed): D_p, the
 *   work matrix and with want_dof C, n_g x n_g fp64 each, allocated for the call and released before it returns.  There is no row
 *   pass, so dazim_map_posterior's LDS bound on n_g does not apply.
 *   Stats: "map_tradeoff" and its parts "map_trade.gram", ".factor", ".solve", ".inverse" (seconds, summed over periods and points),
 *   "map_trade.points" (K), "map_trade.ng", "map_trade.grams" (the Gram passes of the call: kmax, whatever K).
 * dazim_map_tradeoff_total (host only): the criteria of the whole block-diagonal system, for one weight on all periods.  Every total
 *   [K] is the sum over the periods in ascending p (reg2sum_t and dof_t over p and then blk); gcv_t = M chi2_t / (M - dof_t)^2 with
 *   M = sum_p m_p.  dof, logev and their outputs are nullable; a NaN period makes that point's totals NaN. */
int dazim_map_tradeoff(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, const float *b, int nx, int ny, int kmax, int azim, int K,
                       const float *scale, const float *damp, int want_dof, int want_evidence, int64_t *mdata_p, double *chi2,
                       double *reg2, double *xnorm2, double *logdet_a, double *logdet_p, double *dof, double *gcv, double *logev,
                       float *x, int *n_failed);
int dazim_map_tradeoff_total(int K, int kmax, int nblk, const int64_t *mdata_p, const double *chi2, const double *reg2,
                             const double *dof, const double *logev, double *chi2_t, double *reg2sum_t, double *dof_t, double *gcv_t,
                             double *logev_t);

/* dazim_model_posterior: how well the model of the direct 3-D inversion is known, per block (dVs, Gc, Gs), knot and inner cell, from the
 * matrix dazim_lsmr is given in an outer iteration.  The exact regularised solution of that linearised step is
 * what it describes; LSMR stopped at itnlim approximates that solution.
 *   A: the first m_data rows are the weighted data rows (unit variance after dazim_weight_data), the rows after them regularisation
 *   rows of any sparse form (dazim_csr_append_tikhonov's or others); columns in the 3-D layout of dazim_rays_build_G[_joint],
 *   a = blk*maxvp + k*ncell + cell, ncell = (nx-2)(ny-2), maxvp = ncell*(nz-1), n = nblk*maxvp (nblk = 3 with joint, else 1); inside
 *   a row the columns ascend strictly.  damp as given to dazim_lsmr.  One dense block:
 *     D = sum_{data rows} r^T r       P = sum_{regularisation rows} l^T l + damp^2 I       A_n = D + P = R R^T       M = R^-1
 *     C = A_n^-1 = M^T M              Rm = C D = I - C P
 *   std_post, std_noise, rdiag, rsum, width_h, width_z, leak: [nblk][nz-1][ny-2][nx-2] fp32, the layout of dv in dazim_model_update
 *   (host or device):
 *     std_post, std_noise, rdiag, rsum   as dazim_map_posterior defines them
 *     width_h   (nullable) = sqrt(sum_c Rm_ac^2 ((i_c - i_a)^2 + (j_c - j_a)^2) / sum_c Rm_ac^2) over the unknown's own block, all
 *               knots of it, in cells; 0 if the denominator is 0
 *     width_z   (nullable; given together with depz [nz-1], the knots' depths, or both NULL) = sqrt(sum_c Rm_ac^2 (z_c - z_a)^2 /
 *               sum_c Rm_ac^2) over the same entries, in depz's unit; 0 if the denominator is 0
 *     leak      (nullable; NULL unless joint) = the share of sum_c Rm_ac^2 that lies in the other two blocks; 0 if the sum is 0
 *   trace [nblk][nz-1] (nullable) = sum of Rm_aa per block and knot.
 *   rows [nsel][n] (nullable) = row sel[s] of Rm, the point-spread function of unknown sel[s] (what a spike test would show).
 *   Arithmetic, fp64 throughout, every sum in a fixed order, no floating-point atomics, each value rounded to fp32 once:
 *     A_n(a,c) = sum over the rows in ascending row order of r_a r_c (products of the fp32 values in fp64), then damp^2 on the diagonal;
 *     factor, inverse and C are dazim_map_posterior's, by the same kernels (option map_post.mfma selects their tile form);
 *     Rm_ac = delta_ac - sum over the regularisation rows l with l_c != 0 in ascending row order of t_l l_c, then - damp^2 C_ac, with
 *     t_l = sum_e C_ae l_e in ascending e; (Rm C)_aa = sum_c Rm_ac C_ac; a sum along a row: 256 strided partial sums, combined in a
 *     fixed tree.  Host and device arguments give the same bits, and so do two calls.
 *   If the factorisation meets a pivot that is not finite and > 0, every output is NaN and n_failed (host, nullable) is 1, else 0.
 *   Refused (DAZIM_E_BAD_ARG, nothing written): m_data outside 0..m, n not nblk*maxvp, nx or ny < 3, nz < 2, a missing std_post,
 *   std_noise, rdiag or rsum, leak without joint, width_z without depz or the reverse, sel entries outside 0..n-1, rows without sel, a
 *   negative or non-finite damp, a row whose columns do not ascend strictly (found on the device), and a workspace that the card's free
 *   memory cannot hold (the message names the GiB needed): two n x n fp64 matrices, allocated for the call and released before it
 *   returns, and one fp64 per regularisation row for each of the row pass's workgroups.  The matrix's transpose is built if absent.
 *   Stats: "model_posterior" and its parts "model_post.gram", ".factor", ".inverse", ".c", ".rows" (seconds), "model_post.n". */
int dazim_model_posterior(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, int nx, int ny, int nz, int joint, float damp,
                          const float *depz, float *std_post, float *std_noise, float *rdiag, float *rsum, float *width_h,
                          float *width_z, float *leak, int nsel, const int *sel, float *rows, float *trace, int *n_failed);

/* dazim_model_tradeoff: the linearised step of the direct 3-D inversion solved exactly at K regularisation strengths, with what an
 * L-curve, generalised cross-validation and the Bayesian evidence need at each.  A, m_data, nx, ny, nz, joint,
 * the column layout and nblk are dazim_model_posterior's; b [m_data] (host or device) is the weighted right-hand side of the data rows,
 * as dazim_lsmr is given it; the regularisation rows have right-hand side 0.  Every regularisation row lies in one block.
 *   scale [K][nblk], damp [K] (host): point k multiplies the stored regularisation rows of block b by scale[k][b] and damps with damp[k]:
 *     D = sum_{data rows} r^T r     R_b = sum_{regularisation rows of block b} l^T l     g = sum_{data rows} r^T b_r
 *     P_k = sum_b scale[k][b]^2 R_b + damp[k]^2 I        A_k = D + P_k = R R^T        x_k = A_k^-1 g (forward and back substitution)
 *   Outputs (host or device; [K] unless noted):
 *     chi2      |G x_k - b|^2 over the data rows          reg2 [K][nblk]  |L_b x_k|^2, the rows as stored (unscaled)
 *     xnorm2    |x_k|^2                                    logdet_a        2 sum_i log R_ii
 *     logdet_p  (nullable; want_evidence) the same from a second factorisation, of P_k alone; NaN when P_k has a pivot that is not
 *               finite and > 0, which does not count as a failure of the point
 *     dof [K][nblk] (nullable; want_dof)  sum_{a in block b} sum_c C_ac D_ac, C = A_k^-1: block b's share of tr(Rm)
 *     gcv       (nullable; want_dof)      m_data chi2 / (m_data - sum_b dof[b])^2
 *     logev     (nullable; want_evidence) -(chi2 + J)/2 + logdet_p/2 - logdet_a/2 - m_data log(2 pi)/2, J = sum_b scale[k][b]^2 reg2[b]
 *               + damp[k]^2 xnorm2: the log marginal likelihood of b under unit-variance data errors and the prior N(0, P_k^-1)
 *     x [K][n] fp32 (nullable)            x_k, rounded once
 *   A point whose A_k meets a pivot that is not finite and > 0 has NaN in every output and n_failed[k] (host, [K], nullable) = 1, else
 *   0; the other points are not affected.
 *   Arithmetic: fp64, every sum in a fixed order set by the problem alone, no floating-point atomics.  D is formed once per call; at
 *   scale 1 the matrix factored is dazim_model_posterior's, the same numbers added in the same order; the factorisation, and with
 *   want_dof the inverse and C, are its kernels (option map_post.mfma).  Two calls give the same bits, host and device arguments give
 *   the same bits, and a point gives the same bits alone as at any position of any sweep.
 *   Refused (DAZIM_E_BAD_ARG, nothing written): what dazim_model_posterior refuses of A, m_data, nx, ny, nz; K < 1; a missing b, scale,
 *   damp, chi2, reg2, xnorm2 or logdet_a; a negative or non-finite scale or damp; dof or gcv without want_dof; logdet_p or logev
 *   without want_evidence; a regularisation row with entries in two blocks (found on the device); and a workspace the card's free
 *   memory cannot hold (the message names the GiB needed): D, the work matrix and with want_dof C, n x n fp64 each, allocated for the
 *   call and released before it returns.
 *   Stats: "model_tradeoff" and its parts "model_trade.gram" (once per call), ".factor", ".solve", ".inverse" (summed over the points),
 *   ".points", "model_trade.n".
 * dazim_tradeoff_pick (host only): corner = the interior point of largest Menger curvature of the polyline (log chi2, log reg2sum)
 *   through the points where both are finite, in the order given; igcv = the smallest finite gcv; iev = the largest finite logev (gcv,
 *   logev nullable).  An index is -1 when there are fewer than three finite points (corner) or none (igcv, iev). */
int dazim_model_tradeoff(dazim_ctx *ctx, const dazim_csr *A, int64_t m_data, const float *b, int nx, int ny, int nz, int joint, int K,
                         const float *scale, const float *damp, int want_dof, int want_evidence, double *chi2, double *reg2,
                         double *xnorm2, double *logdet_a, double *logdet_p, double *dof, double *gcv, double *logev, float *x,
                         int *n_failed);
int dazim_tradeoff_pick(int K, const double *chi2, const double *reg2sum, const double *gcv, const double *logev, int *corner,
                        int *igcv, int *iev);

/* ---- from the maps to a depth model, cell by cell (the second step of the two-step method) ------------------
 * dazim_vs_kernels: skern [nz][kmax][nx*ny] fp64 = sen_vp*coe_a + sen_rho*coe_rho + sen_vs at vel (the Brocher derivatives of the
 *   cell's velocity, inv/CalSurfG.f90:1339-1364): the table the 3-D rows of dazim_rays_build_G multiply, bit for bit (an iso row
 *   entry of layer k is (float)(skern[k] * (double)fdm)).  vel [nz][ny][nx], sen_* [nz][kmax][nx*ny] from
 *   dazim_dispersion_kernels.
 * dazim_column_lsq: one regularised least-squares problem per inner cell (jj, kk), column jj*nx + kk of the kernel table: for each
 *   right-hand side r, the x that minimises ||diag(w)(K x - r)||^2 + smooth^2 ||L x||^2 + damp^2 ||x||^2, K the cell's kmax x nlay
 *   slice of kern, L the depth rule of TikhRegul (inv/TikhRegul.f90:2) on one column (first and last knot the single entry 2, an
 *   inner knot 2, -1, -1).  fp64 throughout (normal equations, Cholesky), x rounded to fp32.
 *   kern [>= nlay][kmax][nx*ny]: fp64 when kern_fp32 == 0 (skern), fp32 otherwise (Lsen_Gsc); the first nlay layers are read.
 *   rhs [nrhs][kmax][ny-2][nx-2]; wdat [kmax][ny-2][nx-2] = 1/sigma per period and cell, 0 = no data, nullable (all ones).
 *   x out [nrhs][nlay][ny-2][nx-2]: the dv layout of dazim_model_update (nrhs 1: its dVs block; nrhs 2: its Gc and Gs blocks).
 *   A cell whose weights are all 0 gets x = 0 exactly; n_empty (host, nullable) counts those cells.  stats (host, nullable)
 *   [nrhs][kmax][2] = RMS over the cells with w != 0 of r and of r - K x.  Refused (DAZIM_E_BAD_ARG): nlay outside 1..63, kmax
 *   outside 1..60, nrhs not 1 or 2, a negative smooth or damp, smooth == damp == 0.  One launch, one wavefront per cell.     */
int dazim_vs_kernels(dazim_ctx *ctx, int nx, int ny, int nz, int kmax, const float *vel, const double *sen_vs, const double *sen_vp,
                     const double *sen_rho, double *skern);
int dazim_column_lsq(dazim_ctx *ctx, int nx, int ny, int nlay, int kmax, int kern_fp32, const void *kern, int nrhs, const float *rhs,
                     const float *wdat, float smooth, float damp, float *x, int *n_empty, float *stats);

/* dazim_column_resolution: how well dazim_column_lsq's answer is known, per inner cell and knot, from the same Cholesky factor.
 *   kern, kern_fp32, wdat, smooth, damp, nlay, kmax as in dazim_column_lsq.  Per cell, with W = diag(w), L the depth rule:
 *     P = smooth^2 L^T L + damp^2 I      A = K^T W^2 K + P = R R^T      M = R^-1      C = A^-1 = M^T M
 *     Rm = C K^T W^2 K = I - C P         (the resolution matrix: x_est = Rm x_true for noise-free data r = K x_true)
 *   std_post [nlay][ny-2][nx-2]  = sqrt(C_aa): the posterior std when the regulariser is read as a Gaussian prior of precision P
 *                                  and the data errors have std 1/w (the reading of dazim_mc_aniso_result's conditional std)
 *   std_noise                    = sqrt((Rm C)_aa) = sqrt((C K^T W^2 K C)_aa): data errors of std 1/w carried through the
 *                                  estimator alone, <= std_post; summed as sum_p w_p^2 (sum_c C_ac K_pc)^2
 *   rdiag                        = Rm_aa         rsum = sum_c Rm_ac
 *   width                        = sqrt(sum_c Rm_ac^2 (z_c - z_a)^2 / sum_c Rm_ac^2), z = depz [nlay] (host or device); 0 if the
 *                                  denominator is 0.  width and depz are both given or both NULL.
 *   rows [nlay][nlay][ny-2][nx-2] (nullable): rows[a][c] = Rm_ac, row a the averaging kernel of knot a
 *   trace [ny-2][nx-2] (nullable) = sum_a Rm_aa, the number of model parameters the cell's data resolve
 *   C_ac = sum_{i >= max(a, c)} M_ia M_ic in ascending i; C_aa is the (A^-1)(a,a) that dazim_mc_aniso_step adds to avar, bit for
 *   bit.  Rm_ac takes the five C_ae, |e - c| <= 2, in ascending e.  fp64 throughout, every sum in a fixed order, each value rounded
 *   to fp32 once; host and device arguments give the same bits.  A cell whose weights are all 0 gets 0 in every output and is
 *   counted in n_empty; a cell whose factorisation meets a pivot that is not finite and > 0 (non-finite kernels) gets NaN in every
 *   output and is counted in n_failed (both host, nullable).  Refused (DAZIM_E_BAD_ARG): what dazim_column_lsq refuses, a missing
 *   std_post, std_noise, rdiag or rsum, and width without depz or depz without width.  One launch, one wavefront per cell.   */
int dazim_column_resolution(dazim_ctx *ctx, int nx, int ny, int nlay, int kmax, int kern_fp32, const void *kern, const float *wdat,
                            float smooth, float damp, const float *depz, float *std_post, float *std_noise, float *rdiag, float *rsum,
                            float *width, float *rows, float *trace, int *n_empty, int *n_failed);

/* ---- radial anisotropy: Vsv from the Rayleigh maps, Vsh from the Love maps, cell by cell -------------------
 * dazim_column_lsq_radial: per inner cell the updates x = [xv; xh] of the Vsv and the Vsh knots (nlay each, N = 2 nlay) that minimise
 *     ||Wv (Kv xv - rv)||^2 + ||Wh (Kh xh - rh)||^2 + smooth^2 (||L xv||^2 + ||L xh||^2) + damp^2 ||x||^2
 *       + couple^2 ||xh - xv + d0||^2
 *   Kv [kv][nlay] the cell's slice of kern_v (dazim_vs_kernels of the Vsv model over the Rayleigh periods), Kh [kh][nlay] that of
 *   kern_h (the Vsh model over the Love periods), L the depth rule of dazim_column_lsq, d0 the current Vsh - Vsv at the knots: the
 *   smoothing and the damping act on the update, the coupling on the model.  Normal equations, with m2 = couple^2 and
 *   P = smooth^2 L^T L + damp^2 I:
 *     A = [[Kv^T Wv^2 Kv + P + m2 I, -m2 I], [-m2 I, Kh^T Wh^2 Kh + P + m2 I]] = R R^T
 *     b = [Kv^T Wv^2 rv + m2 d0; Kh^T Wh^2 rh - m2 d0]
 *   kern_v [>= nlay][kv][nx*ny], kern_h [>= nlay][kh][nx*ny] fp64, NULL exactly when the count is 0; rhs_v, rhs_h and w_v, w_h
 *   [kv | kh][ny-2][nx-2] (w = 1/sigma, 0 = no data, NULL = all ones); d0 [nlay][ny-2][nx-2] (NULL = 0).
 *   x out [2][nlay][ny-2][nx-2]: dVsv, then dVsh, each a dVs block of dazim_model_update.  A cell without a non-zero weight in
 *   either block gets x = 0 exactly and is counted in n_empty (host, nullable); a cell with data in one block only is solved, and
 *   with couple > 0 the other profile follows through the coupling.  stats (host, nullable) [kv + kh][2] as dazim_column_lsq's, the
 *   Rayleigh periods first.  With couple = 0 each block goes through the operations of dazim_column_lsq on that block alone.
 * dazim_column_resolution_radial: how well that answer is known, from the same factor.  With
 *   P2 = [[P + m2 I, -m2 I], [-m2 I, P + m2 I]], M = R^-1, C = A^-1 = M^T M and Rm = I - C P2 (x_est = Rm x_true for noise-free data
 *   and d0 = 0), index a = blk*nlay + knot (blk 0 Vsv, 1 Vsh):
 *     std [2][nlay][ny-2][nx-2]   = sqrt(C_aa)            cov_vh [nlay][ny-2][nx-2] = C_{a, nlay + a}, the Vsv-Vsh covariance of a knot
 *     rdiag [2][nlay][..]         = Rm_aa                 rsum [2][nlay][..] = sum over all 2 nlay columns of Rm_ac
 *     cross [2][nlay][..]         = sum_{c in the other block} |Rm_ac| / sum_{all c} |Rm_ac|: the share of the knot's averaging kernel
 *                                   that lies in the other profile; 0 if the denominator is 0
 *     trace [2][ny-2][nx-2] (nullable) = sum_a Rm_aa per block      rows [2 nlay][2 nlay][ny-2][nx-2] (nullable): rows[a][c] = Rm_ac
 *   M_ij = -(sum_{l = j+1..i} M_il R_lj) / R_jj in ascending l; C_ac = sum_{i >= max(a, c)} M_ia M_ic in ascending i; Rm_ac takes the
 *   five entries of P + m2 I in c's block in ascending order, then -m2 at c's knot in the other block.  A cell without data gets 0 in
 *   every output (n_empty), a cell with a pivot that is not finite and > 0 NaN in every output (n_failed; both host, nullable).
 * Both: fp64 throughout, every sum in a fixed order, each value rounded to fp32 once; host and device arguments give the same bits.
 *   Refused (DAZIM_E_BAD_ARG): nlay outside 1..63, kv < 0, kh < 0, kv + kh outside 1..60, a negative smooth, damp or couple,
 *   smooth == damp == 0 (A would not be definite whatever couple is), a kernel table missing for a count that is not 0 or given for a
 *   count of 0, a missing right-hand side, a missing x, std, cov_vh, rdiag, rsum or cross.  One launch, one workgroup per cell
 *   (64 lanes up to nlay = 32, 128 beyond), A as a packed lower triangle in LDS: 8 (N (N + 1) / 2 + (kv + kh)(nlay + 2) + N) bytes,
 *   96 216 at nlay = 63, kv + kh = 60.                                                                                             */
int dazim_column_lsq_radial(dazim_ctx *ctx, int nx, int ny, int nlay, int kv, const double *kern_v, int kh, const double *kern_h,
                            const float *rhs_v, const float *rhs_h, const float *w_v, const float *w_h, const float *d0, float smooth,
                            float damp, float couple, float *x, int *n_empty, float *stats);
int dazim_column_resolution_radial(dazim_ctx *ctx, int nx, int ny, int nlay, int kv, const double *kern_v, int kh, const double *kern_h,
                                   const float *w_v, const float *w_h, float smooth, float damp, float couple, float *std,
                                   float *cov_vh, float *rdiag, float *rsum, float *cross, float *trace, float *rows, int *n_empty,
                                   int *n_failed);

/* ---- Monte-Carlo Vs per map cell: posterior mean, spread and credible interval ----------------------------
 * Random-walk Metropolis chains on the knots 0..nlay-1 (nlay = nz - 1) of each inner cell's Vs column, the last knot held at vel0's
 * value; the forward model is dazim_dispersion_kernels with sen_* = NULL.  Prior: uniform on [vmin, vmax] per cell and knot.
 * chi^2 = sum_p (w_p (cobs_p - c_p))^2 in period order in fp64 ((double)w * ((double)cobs - c), periods with w == 0 skipped);
 * c_p == 0 at a period with w != 0 (no root) gives chi^2 = +inf.  Cells with w == 0 at every period are not sampled (n_empty).
 * Sampled cells are the others in inner-cell order (cs = 0, 1, ..); chain ch of sampled cell cs is column cs*nchain + ch (ncol =
 * sampled cells * nchain).  Global chain id gid = cell*nchain + ch, cell = (jj-1)(nx-2) + kk-1 the index among ALL inner cells.
 * Random numbers, all in fp64: block(step, gid, b) = the four words of Philox4x32-10 with counter (step, gid, b, 0) (32-bit words,
 *   first word first; step truncated to 32 bits) and key (seed & 0xffffffff, seed >> 32); u(word) = (word + 0.5) * 2^-32.
 *   Start models (step 0): knot 4q+e = (float)(lo + (hi - lo) * u(word e of block(0, gid, 1+q))), lo/hi = (double)vmin/vmax.
 *   Normals of step t: from block(t, gid, 1+q) = (w0, w1, w2, w3): r0 = sqrt(-2 log u(w0)), a0 = 6.283185307179586 * u(w1),
 *   r1, a1 likewise from w2, w3; knots 4q, 4q+1, 4q+2, 4q+3 get r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1.
 *   Acceptance uniform of step t: u(word 0 of block(t, gid, 0)).
 * Step t (t = 1, 2, ..; a dazim_mc_step call, or one step of dazim_mc_run), per chain:
 *   chi2' from the curves pv [kmax][ncol] of the proposals.  t = 1: the proposals are the start models; they become the state with
 *   chi2', no decision.  t > 1: current chi2 = +inf -> accept iff chi2' is finite; else accept iff log(u) < -0.5 * (chi2' - chi2).
 *   An accepted proposal replaces the state's nlay knots and chi2.
 *   Burn-in (record = 0): the cell's accepted moves are counted over its chains; after every nadapt burn-in steps with a decision,
 *   rate = count / (nadapt * nchain): > 0.40 -> s = s * 1.25f, < 0.20 -> s = s / 1.25f, then s = min(max(s, 1e-3f), 0.5f) (fp32),
 *   and the count restarts.  Recorded steps (record = 1) keep s: per chain and knot sums[0][k][col] += v, sums[1][k][col] += v*v
 *   (fp64, v the state); hist[cs][k][b] += 1, b = (int)(((double)v - lo) / (hi - lo) * nbin) clamped to 0..nbin-1; accepted[col]
 *   += 1 for an accepted move; the cell's best model is the state of its lowest-chi2 chain when that chi2 is strictly lower than
 *   the best so far (the first in (step, chain) order on ties).
 *   Next proposals: v' = (double)v + ((double)s * (hi - lo)) * z_k, reflected (v' < lo -> 2 lo - v', v' > hi -> 2 hi - v') until
 *   inside, rounded to fp32 once; the last knot stays.  (|z| < 6.77 and s <= 0.5 bound the excess by 3.39 widths: at most 4
 *   reflections.  The loop stops after 8 and clamps to the box, which never acts.)
 * Proposal kind 1 (dazim_mc_set_proposal; kind 0 is the step above, unchanged): the proposal takes the shape of the chains' own
 *   covariance, learnt during burn-in (Haario et al., 2001) and frozen afterwards: the recorded steps are plain Metropolis steps with
 *   a fixed symmetric proposal.  Per sampled cell, with npair = nlay (nlay + 1) / 2 and pair (a, c), c <= a, at a (a + 1) / 2 + c, the
 *   handle holds cov_n (int64), cov_s1 [nlay], cov_s2 [npair] (fp64), chol [npair] (fp64, a lower-triangular factor) and cov_set
 *   (int), all 0 at the start.  The step gains:
 *   Accumulate: in a burn-in step with a decision (record = 0, t > 1), after the decision, for the chains ch = 0 .. nchain-1 in that
 *   order, with u_k = ((double)v_k - lo_k) / (hi_k - lo_k) of the chain's state: cov_s1[k] += u_k, cov_s2[(a,c)] += u_a * u_c,
 *   cov_n += 1.  Recorded steps accumulate nothing.
 *   Factor: at the end of an adaptation window, after the scale rule, nothing if cov_n < 8 nlay (the sums keep growing: windows
 *   merge for few chains).  Otherwise m = s1 / n, C(a,c) = s2(a,c) / n - m_a * m_c, the diagonal + 1e-8; a right-looking Cholesky in
 *   dazim_column_lsq's elimination order (column by column: pivot p = C(c,c), d = sqrt(p), the column below / d, then one update
 *   C(a,e) -= C(a,c) * C(e,c) per element of the trailing triangle) in fp64, stopped at the first pivot that is not finite and > 0.
 *   If no pivot stopped it chol takes the factor, and if cov_set was 0 it becomes 1 and the cell's s becomes 1.0f / sqrtf((float)
 *   nlay); otherwise chol and cov_set stay.  In both cases cov_n, cov_s1 and cov_s2 return to 0.
 *   Scale range: while cov_set is 1 (as the scale rule finds it, before this window's factor) the clamp of s is [1e-3f, 2.0f /
 *   sqrtf((float)nlay)] (fp32) instead of [1e-3f, 0.5f]; the thresholds and the factor 1.25f are the same.
 *   Next proposals, same normals z: where cov_set is 1, y_k = sum_{j=0..k} chol(k,j) * z_j summed in j order in fp64 and v' =
 *   (double)v + ((double)s * (hi - lo)) * y_k, with the same reflections, one rounding to fp32 and the last knot untouched; where
 *   cov_set is 0, the formula above.  (u in [0, 1] bounds C_kk, the squared norm of row k of chol, by 1/4 + 1e-8; each Box-Muller
 *   pair has norm <= 6.77, so |z|_2 <= 6.77 sqrt(ceil(nlay / 2)); s <= 2 / sqrt(nlay): the excess stays below 6.78 widths, at most 7
 *   reflections, and the clamp still never acts.)
 * Parallel tempering (dazim_mc_set_tempering; without it, or with ntemp = 1, the step is the one above, unchanged): replica exchange
 *   (Swendsen and Wang, 1986; Geyer, 1991) for posteriors with separate modes.  ntemp divides nchain; chain ch is rung r = ch % ntemp
 *   of replica group g = ch / ntemp, so ncold = nchain / ntemp chains (ch = 0, ntemp, 2 ntemp, ..) sit at rung 0.  beta_0 = 1 and
 *   beta_r = tmax^(-r / (ntemp - 1)) (pow in fp64 on the host, once; the step takes beta from the handle); rung r samples the
 *   posterior to the power beta_r, rung 0 the posterior itself.  Per sampled cell the handle holds scale and its window count per
 *   rung [ntemp] (every scale starts at dazim_mc_create's step) and swap_try, swap_acc [ntemp - 1] (int64, 0 at the start).  The
 *   step changes in this way:
 *   Decision at rung r: accept iff log(u) < -0.5 * beta_r * (chi2' - chi2) (fp64, evaluated left to right); the uniform, the t = 1
 *   rule and the rules for chi2 = +inf are the ones above.
 *   Scale: rung r of a cell counts the accepted burn-in moves of its ncold chains; at the end of a window rate_r = count_r / (nadapt *
 *   ncold) moves the rung's own scale with the thresholds, the factor 1.25f and the clamps above ([1e-3f, 2.0f / sqrtf((float)nlay)]
 *   for every rung while the cell's cov_set is 1), and every rung's count restarts.  dazim_mc_state's scale is rung 0's.
 *   Swap: in a step with a decision (t > 1) and t % nswap == 0, after the decision and before anything is recorded, accumulated or
 *   proposed; round w = t / nswap pairs the rungs (r, r + 1) with r % 2 == w % 2 and r + 1 < ntemp in every group.  For the pair of
 *   chain cl (rung r) and cl + 1: u = u(word 1 of block(t, gid(cl), 0)), D = 0.5 * (beta_r - beta_{r+1}) * (chi2_r - chi2_{r+1})
 *   (fp64, left to right).  Both chi2 finite: swap iff log(u) < D.  chi2_r = +inf and chi2_{r+1} finite: swap.  Otherwise no swap.
 *   A swap exchanges the two chains' nlay knots and chi2; the last knot stays.  swap_try[r] += 1 per pair of the round, swap_acc[r]
 *   += 1 per swap, over the groups and over all steps.
 *   Records: only the rung-0 chains add to sums, hist and accepted (the columns of the other chains stay 0); the best model is the
 *   lowest chi2 over all chains of the cell after the swap, with the tie rule above.  dazim_mc_result takes the ncold rung-0 chains
 *   in chain order with M = ncold everywhere (R-hat NaN for ncold = 1; accept = their accepted moves / (decisions * ncold)).
 *   Kind 1: the sums take the states of the rung-0 chains only, after the swap, in chain order, and cov_n += ncold; the 8 nlay rule,
 *   the factor and the reset are unchanged.  A cell has one factor, used by every rung with the rung's own scale, and at the first
 *   factor every rung's scale becomes 1.0f / sqrtf((float)nlay).  The clamps of s being the same, the bounds on the number of
 *   reflections above hold at every rung.
 *   Next proposals: the formulas above with s the scale of the chain's rung.
 * Gc/Gs posteriors (dazim_mc_set_aniso; without it, or with nthin = 0, every launch and every result is the one above, unchanged):
 *   the 2-psi terms a1, a2 of a cell are linear in Gc/L, Gs/L, so conditional on one Vs column their posterior
 *   under Gaussian data errors and dazim_column_lsq's quadratic regulariser is Gaussian with mean x^(Vs) = dazim_column_lsq's solution
 *   and covariance C(Vs) = the inverse of its normal matrix.  Averaging both over thinned states of the rung-0 chains gives the
 *   marginal: mean = E[x^], Var = E[diag C] + Var[x^]; the second term is the share of the Vs uncertainty.  Nothing is sampled.
 *   Notation: ncold = nchain / ntemp, ncolc = sampled cells * ncold; rung-0 chain g of sampled cell cs is cold column cs*ncold + g,
 *   chain ch = g*ntemp, column cs*nchain + ch of the handle.
 *   dazim_mc_set_aniso: amap [2][kmax][ny-2][nx-2] = a1 then a2 (the rhs layout of dazim_column_lsq with nrhs = 2), wa [kmax][ny-2]
 *   [nx-2] = 1/sigma_a per period and cell, 0 = no data (host or device); smooth, damp as in dazim_column_lsq.  nthin >= 1 switches
 *   the sums on, nthin = 0 restores the default (the arrays are not looked at then).  It may come before or after
 *   dazim_mc_set_proposal and dazim_mc_set_tempering; ntemp is the handle's when the first sample is taken.  The handle then holds,
 *   all 0: asum [5][nlay][ncolc] fp64 (sums of xc, xs, xc^2, xs^2, xc*xs), avar [nlay][ncolc] fp64 (sum of diag C), acnt [ncolc] int64
 *   and the count skipped (int64; kept per cold column and added up when it is asked for).  DAZIM_E_BAD_ARG for nthin < 0, a
 *   non-finite amap or wa, a negative smooth or damp, smooth == damp == 0, a handle of another context, or once a step has been done.
 *   dazim_mc_aniso_step: one sample from the chains' current states.  lsen [nlay][kmax][ncolc] fp32 (host or device) = Lsen_Gsc of
 *   the cold columns' states, what dazim_ti_kernels writes for nx = ncolc, ny = 1; from any source, as dazim_mc_step's curves.  A
 *   cold column whose chain has chi2 = +inf is skipped: skipped += 1, nothing else.  For every other cold column, K its kmax x nlay
 *   slice of lsen, w, r1, r2 its cell's wa and amap, s2 = (double)smooth^2, d2 = (double)damp^2, all in fp64:
 *     w2_p = (double)w_p * (double)w_p, wr_rp = w2_p * (double)r_rp (0 where w_p == 0);
 *     A(a,c) = sum_p w2_p * K(p,a) * K(p,c) (p order, left to right, periods with w2_p == 0 left out), + s2 * (L^T L)(a,c), + d2 when
 *     a == c; b_r(a) = sum_p wr_rp * K(p,a) likewise: dazim_column_lsq's sums in its order (one device function serves both).
 *     Its right-looking Cholesky A = R R^T (column c: d = sqrt(A(c,c)), the column below / d, then A(a,e) -= A(a,c) * A(e,c) on the
 *     trailing triangle) and its two substitutions give xc, xs, kept in fp64.
 *     Column k of R^-1: y_k = 1 / R(k,k), y_i = -(sum_{j=k..i-1} R(i,j) * y_j) / R(i,i) for i > k, the sum in j order;
 *     (A^-1)(k,k) = sum_{i>=k} y_i^2 in i order.
 *     asum[0..4][k][col] += xc_k, xs_k, xc_k^2, xs_k^2, xc_k * xs_k; avar[k][col] += (A^-1)(k,k); acnt[col] += 1.
 *   A row of K that is all 0 (dazim_ti_kernels writes one where the state's curve has no root) adds nothing to A or b.  A pivot that
 *   is not finite and > 0 cannot occur with smooth > 0 or damp > 0 and finite inputs; if one does the column is skipped and counted,
 *   nothing is added.  DAZIM_E_BAD_ARG before the handle's first step, when Gc/Gs is not switched on, for a kmax or ncolc that is
 *   not the handle's, for a handle of another context.
 *   dazim_mc_aniso_state: nthin, and copies (each nullable, host or device; skipped host) of asum, avar, acnt and skipped.
 *   DAZIM_E_BAD_ARG when Gc/Gs is off and an array is requested.
 *   dazim_mc_aniso_result, per sampled cell, every sum over its cold columns in column order inside one lane, fp64: n = sum acnt,
 *   S_e = sum asum[e], Sv = sum avar; m_c = S_0 / n, m_s = S_1 / n, between_c = max(S_2 / n - m_c^2, 0), between_s likewise from S_3,
 *   within = Sv / n.  mean [2][nlay][ny-2][nx-2] = m_c then m_s, std = sqrt(within + between), std_between = sqrt(between) (both
 *   [2][nlay][ny-2][nx-2]), cov_cs [nlay][ny-2][nx-2] = S_4 / n - m_c * m_s, nsamp [ny-2][nx-2] (int64) = n; each rounded to fp32
 *   once.  Cells without Vs data: all 0.  A sampled cell with n = 0: mean 0, std, std_between and cov_cs NaN.  Refused before the
 *   first sample.
 *   dazim_mc_run with Gc/Gs on: after every recorded step whose count over the handle's life is a multiple of nthin, one pass: the
 *   rung-0 states into a compact [nz][ncolc] table, dazim_dispersion_kernels on it (nx = ncolc, ny = 1, curves only, a curve buffer
 *   of its own), dazim_ti_kernels on the same columns, then the sample above.  Where the TI scratch of all cold columns would pass
 *   2 GiB the pass goes through the columns in blocks of whole cells (option "mc.aniso_block_cells" > 0 sets the cells per block);
 *   every column's arithmetic is its own, so the results do not depend on the blocks.  The pass reads the chains and writes only
 *   its own arrays: the Vs chain, its records and its random numbers are bit for bit what they are without it.  Stats: "mc.aniso"
 *   (seconds of the run's passes), "mc.aniso_passes", "mc.aniso_skipped" (0 when Gc/Gs is off).
 * Hierarchical data noise (dazim_mc_set_noise; without it, or with a0 = 0, every launch and every result is the one above,
 *   unchanged): the noise level becomes an unknown of the posterior (Bodin et al., 2012) and is integrated out in closed form, so no
 *   random number and no tuning knob is added.
 *   Noise model: the data std of period p in a cell is lambda / w_p, lambda one unknown factor per cell and chain, with the prior
 *   lambda^2 ~ InverseGamma(a0, b0).  Per sampled cell nd = the number of periods with w != 0 (the same for all of its chains),
 *   a = (double)a0 + 0.5 * nd, B(chi2) = (double)b0 + 0.5 * chi2.  Integrating lambda out of lambda^-nd exp(-chi2 / (2 lambda^2))
 *   p(lambda^2) leaves a marginal posterior of the knots proportional to B(chi2)^-a inside the box (a Student-t in the residuals).
 *   Energy: X(chi2) = 2.0 * a * log(B(chi2)) in fp64, X(+inf) = +inf.
 *   Step: the one above with X in place of chi2 wherever a decision is taken, nothing else: accept iff log(u) < -0.5 * (X' - X),
 *   tempered log(u) < -0.5 * beta_r * (X' - X), swap D = 0.5 * (beta_r - beta_{r+1}) * (X_r - X_{r+1}), each evaluated left to right
 *   as the formulas above are written; the rules for +inf are the ones above.  The uniforms, the normals and the proposals,
 *   reflection and scale adaptation, the covariance sums and factor, the records of Vs, the histogram and the best model (lowest raw
 *   chi2; X is monotone in it) stay what they are, and the handle still stores raw chi2 in chi2, best_chi2 and chi2_best.
 *   Noise record: at a recorded step, after the decision and any swap, a chain at rung 0 whose chi2 is finite adds, with B at its
 *   state, nsum[0][col] += sqrt(B), nsum[1][col] += B (fp64) and ncnt[col] += 1 (int64); a chain at +inf adds nothing.  nsum
 *   [2][ncol] and ncnt [ncol] are 0 at the start, and the columns of the other rungs stay 0.
 *   Result (dazim_mc_noise_result): conditional on a state lambda^2 ~ IG(a, B), so E[lambda] = g E[sqrt(B)] with g = Gamma(a - 1/2)
 *   / Gamma(a) and E[lambda^2] = E[B] / (a - 1).  One lane per inner cell, the sums over its cold columns in column order in fp64:
 *   n = sum ncnt, S0 = sum nsum[0], S1 = sum nsum[1]; g = exp(lgamma(a - 0.5) - lgamma(a)) from a table over nd = 0..60 that the
 *   host makes once when the mode is set; lam_mean = g * S0 / n, lam_std = sqrt(max(S1 / (n * (a - 1)) - lam_mean^2, 0)), NaN where
 *   a <= 1; both NaN for n = 0; cells without data get 0; each rounded to fp32 once.  ndata [ny-2][nx-2] (int32) = nd.
 *   The Gc/Gs sums of dazim_mc_set_aniso are unchanged by the mode: they keep 1/sigma_a and do not see lambda.  Both modes may be
 *   on together.  Stat "mc.noise" of dazim_mc_run is 0 or 1.
 *   dazim_mc_set_noise: a0 > 0 switches the mode on with the prior (a0, b0); a0 == 0 restores the default (b0 is not looked at
 *   then).  It may come before or after dazim_mc_set_proposal, dazim_mc_set_tempering and dazim_mc_set_aniso.  DAZIM_E_BAD_ARG for
 *   a non-finite or negative a0, for a0 > 0 with b0 not finite or <= 0, for a handle of another context, or once a step has been
 *   done.
 *   dazim_mc_noise_state: a0, b0 (0, 0 while the mode is off) and copies of nsum and ncnt (each pointer nullable, the arrays host or
 *   device).  DAZIM_E_BAD_ARG when the mode is off and an array is requested.
 *   dazim_mc_noise_result: lam_mean, lam_std [ny-2][nx-2] fp32 and ndata [ny-2][nx-2] int32 (host or device).  Refused with the
 *   mode off or before the first recorded step.
 * One noise scale per group of periods (dazim_mc_set_noise_groups; one group is dazim_mc_set_noise itself, the same kernel and the
 *   same bits): joint data of several wave types do not share a noise level, so every period p is given a group grp[p] in 0..G-1,
 *   G <= 4, and the data std of period p in a cell is lambda_g / w_p, g = grp[p], lambda_g^2 ~ InverseGamma(a0_g, b0_g), the groups
 *   independent a priori.  Each lambda_g integrates out as above, which is exact: the likelihood factorises over the groups.
 *   Per sampled cell nd_g = the periods of group g with w != 0, a_g = (double)a0_g + 0.5 * nd_g.  Per chain, beside chi2 (the total,
 *   the one sum over all periods in period order as above, unchanged), chi2_g = the same terms summed per group, each in period
 *   order from 0.0; a period with data and no root makes chi2 and its group's chi2_g +inf.  B_g = (double)b0_g + 0.5 * chi2_g.
 *   Energy: X = sum over g = 0..G-1 in that order from 0.0, over the groups with nd_g > 0, of 2.0 * a_g * log(B_g), fp64; X = +inf
 *   where chi2 = +inf.  Step: the hierarchical one above with this X (and E = X under the smoothness prior); the rules for +inf still
 *   test the total chi2.  The handle keeps the chi2_g of every chain's state in chi2g [G][ncol] (+inf before the first step); an
 *   accepted proposal stores its chi2_g and a swap exchanges them with the knots and chi2.  chi2, best, best_chi2 keep their meaning.
 *   Noise record: a recorded rung-0 chain with finite chi2 adds, for every g with nd_g > 0, nsum[0][g][col] += sqrt(B_g) and
 *   nsum[1][g][col] += B_g, and ncnt[col] += 1; nsum is [2][G][ncol].
 *   Result (dazim_mc_noise_groups_result), one lane per (group, inner cell), as dazim_mc_noise_result with the group's a_g, sums and
 *   table row: lam_mean, lam_std [G][ny-2][nx-2] fp32 and ndata [G][ny-2][nx-2] int32 = nd_g; 0 for a cell without data and for a
 *   group without data in a sampled cell, NaN where nothing was recorded, lam_std NaN where a_g <= 1.
 *   Stat "mc.noise" of dazim_mc_run is 2 with G >= 2 groups, and "mc.noise_groups" is G (0 off, 1 for dazim_mc_set_noise).
 *   dazim_mc_set_noise_groups: ngroup in 1..4, group_of_period [kmax] in 0..ngroup-1, a0, b0 [ngroup], host arrays.  Every a0 == 0
 *   restores the default.  DAZIM_E_BAD_ARG for ngroup outside 1..4, a group index out of range, a non-finite or negative a0, a0 zero
 *   for some groups and positive for others, a positive a0 with b0 not finite or <= 0, or once a step has been done.  While G >= 2
 *   groups are on, dazim_mc_noise_state gives a0 = b0 = 0 and dazim_mc_noise_result is refused.
 *   dazim_mc_noise_groups_state: ngroup (0 while no noise mode is on) and copies of group_of_period [kmax], a0, b0 [ngroup] (host),
 *   chi2g [ngroup][ncol] (one group: chi2 itself), nsum [2][ngroup][ncol], ncnt [ncol] (each nullable; host or device unless stated).
 *   DAZIM_E_BAD_ARG when no mode is on and an array is requested.
 * Typed data (dazim_mc_set_segments; without it, or with the one segment (2, 0), every launch and every result is the one above,
 *   unchanged): the handle's kmax periods are the virtual periods of nseg segments laid end to end, segment s being seg_kmax[s]
 *   periods of wave seg_iwave[s] (1 Love, 2 Rayleigh) and velocity seg_igr[s] (0 phase, 1 group), under the rules of
 *   dazim_dispersion_kernels_typed (host arrays, nseg in 1..4, no type twice); the lengths sum to kmax.  dazim_mc_run then computes
 *   the proposals' curves with dazim_dispersion_kernels_typed (curves only, nx = ncol, ny = 1, device arrays), "mc.disp" summing
 *   the seconds of both dispersion timers.  The step itself does not look at the type of a period.  Refused once a step has been
 *   done.  The Gc/Gs kernel Lsen_Gsc is Rayleigh-phase: dazim_mc_set_aniso on a handle with other segments, and other segments on a
 *   handle with Gc/Gs on, are refused.
 * Gaussian smoothness prior (dazim_mc_set_prior; without it, or with smooth = damp = 0, every launch and every result is the one
 *   above, unchanged): dazim_column_lsq's regulariser read as the prior that dazim_column_resolution reads it as, a Gaussian of
 *   precision P = smooth^2 L^T L + damp^2 I about a reference column vref, so that the chains' spread means what std_post means and
 *   the directions the data do not determine become proper.  The uniform box stays: it truncates the Gaussian, and the start models
 *   are still the box draws.
 *   Prior energy of a column's fp32 knots v_0..v_{nlay-1} (the fixed last knot takes no part), all in fp64 without contraction:
 *   s2 = (double)smooth * (double)smooth, d2 likewise; d_k = (double)v_k - (double)vref_k; t_a = 2.0 * d_a for a == 0 or a == nlay-1,
 *   else t_a = (2.0 * d_a - d_{a-1}) - d_{a+1} (the L of dazim_column_lsq); q1 = sum_a t_a * t_a and q2 = sum_a d_a * d_a, both in
 *   ascending a from 0.0; Q = s2 * q1 + d2 * q2.  exp(-Q / 2) is the Gaussian of precision P.
 *   Step: the one above with E + Q in place of E wherever a decision is taken, E = chi2 or, in noise mode, X(chi2); lambda is not
 *   applied to the prior.  Accept iff log(u) < -0.5 * beta_r * ((E' + Q') - (E + Q)), Q' of the proposal and Q of the state; swap
 *   D = 0.5 * (beta_r - beta_{r+1}) * ((E_r + Q_r) - (E_{r+1} + Q_{r+1})) with the Q of the states after the decision, and a swap
 *   exchanges them with the knots: rung r samples (likelihood x Gaussian prior)^beta_r.  The rules for +inf still test chi2 alone.
 *   The uniforms, the normals, the proposals and their reflection, the scale and covariance adaptation, the records, the histogram,
 *   the noise record and the Gc/Gs pass do not change, and the handle still stores raw chi2.  The best model stays the state of
 *   lowest raw chi2: the best-fitting model, not the maximum a posteriori.  Stat "mc.prior" of dazim_mc_run is 0 or 1.
 *   dazim_mc_set_prior: smooth, damp as in dazim_column_lsq; vref [nlay][ny-2][nx-2] (host or device), NULL = vel0's knots.  smooth
 *   == 0 and damp == 0 restore the default (vref is not looked at then).  It may come before or after the other dazim_mc_set_*
 *   calls.  DAZIM_E_BAD_ARG for a negative or non-finite smooth or damp, a non-finite vref, a handle of another context, or once a
 *   step has been done.
 *   dazim_mc_prior_state: smooth, damp (0, 0 while the prior is off) and copies of vref and of q [ncol], the Q of the chains' current
 *   states (each pointer nullable, the arrays host or device).  DAZIM_E_BAD_ARG when the prior is off and an array is requested.
 * Radial anisotropy (dazim_mc_set_radial; without it every launch and every result is the one above, unchanged): the handle's knots
 *   are read as the stacked vector [Vsv_0..Vsv_{n-1}, Vsh_0..Vsh_{n-1}, deepest], nlay = 2n <= 62, of dazim_column_lsq_radial:
 *   dazim_mc_create is called with nz = 2n + 1, vel0 [2n+1][ny][nx] the Vsv start knots, then the Vsh start knots, then the one
 *   deepest knot both profiles keep, vmin / vmax [2n][ny-2][nx-2] likewise.  The step does not ask what a knot means: the draws, the
 *   proposals, the covariance sums and factor (which pick up the Vsv-Vsh correlation), the ladder, the noise groups, sums, hist and
 *   R-hat are the ones above on 2n knots.  What changes:
 *   Forward model (dazim_mc_run; depz has n + 1 entries): the physics of dazim_column_lsq_radial with the same neglect of the
 *   cross-sensitivities.  Per step two dazim_dispersion_kernels_typed calls, curves only, nx = ncol, ny = 1, nz = n + 1: the
 *   Rayleigh segments (the first ones, kR periods) on the Vsv model [n+1][ncol] into rows [0, kR) of the curves, the Love segments on
 *   the Vsh model into rows [kR, kmax).  The Vsh model is rows n..2n of the proposals as they lie; the Vsv model is an array of the
 *   handle's that holds the Vsv knots beside a copy of the deepest row: the step stores every proposed Vsv knot to both, so there is
 *   no copy and no host wait between a step and the next dispersion call.  dazim_mc_radial_models hands out both device arrays (the
 *   ones the run's calls read; valid after dazim_mc_set_radial and after every step).  "mc.disp" sums both calls, n_no_root counts a
 *   proposal whose Rayleigh or Love curve has no root once; stat "mc.radial" is 1.
 *   Prior: with d = v - vref per profile, Q = s2 (|L dv|^2 + |L dh|^2) + d2 (|dv|^2 + |dh|^2) + m2 |vh - vv|^2, the precision
 *   [[P + m2 I, -m2 I], [-m2 I, P + m2 I]] of dazim_column_resolution_radial (the coupling on the model, the rest about vref); s2, d2
 *   from dazim_mc_set_prior, whose vref is [2n][ny-2][nx-2], m2 = (double)couple * (double)couple.  Sum order, fp64, no contraction:
 *   q1 = q2 = 0.0; for the profile of Vsv (knots k0 = 0) and then of Vsh (k0 = n), for a = 0..n-1: d_a = (double)v_{k0+a} - (double)
 *   vref_{k0+a}, t_a = 2.0 * d_a for a == 0 or a == n-1, else (2.0 * d_a - d_{a-1}) - d_{a+1} (L inside the profile: no row crosses
 *   the boundary), q1 += t_a * t_a, q2 += d_a * d_a; then qc = 0.0 and for a = 0..n-1: c_a = (double)v_{n+a} - (double)v_a, qc +=
 *   c_a * c_a; Q = (s2 * q1 + d2 * q2) + m2 * qc.  The prior path (E + Q, above) is on when any of smooth, damp, couple is non-zero;
 *   dazim_mc_set_prior and dazim_mc_set_radial give the same Q of the start models in either order, and with smooth = damp = 0 vref
 *   stays what it was (vel0's knots where there was none).
 *   Record: a recorded rung-0 chain adds, per knot pair a < n of its state after the decision and any swap, with vv = (double)v_a,
 *   vh = (double)v_{n+a}, r = vh / vv, xi = r * r, V = sqrt((2.0 * vv * vv + vh * vh) / 3.0) (the Voigt average): rsum[0..4][a][col]
 *   += xi, xi * xi, vv * vh, V, V * V (fp64); ngt1[a][col] += 1 where xi > 1.0 (int64); xhist[cs][a][b] += 1, b = (int)((xi - lo) /
 *   (hi - lo) * nbin) clamped to 0..nbin-1 over the pair's exact range lo = rl * rl, rl = (double)vmin_{n+a} / (double)vmax_a, hi =
 *   rh * rh, rh = (double)vmax_{n+a} / (double)vmin_a.  All 0 at the start; the columns of the other rungs stay 0.
 *   dazim_mc_set_radial: couple = mu >= 0 (1 / the std of Vsh - Vsv; 0 = no coupling).  DAZIM_E_BAD_ARG once a step has been done,
 *   when nz - 1 is odd, for a negative or non-finite couple, unless dazim_mc_set_segments has given at least one Rayleigh and one
 *   Love segment with every Rayleigh segment before every Love segment (later dazim_mc_set_segments calls are held to the same),
 *   on a handle with dazim_mc_set_aniso on (and dazim_mc_set_aniso is refused on a radial handle), and when any vmin is <= 0 (xi
 *   would have no range).  A radial handle stays radial.
 *   dazim_mc_radial_state: n (0 on a handle that is not radial), couple, and copies of rsum [5][n][ncol], ngt1 [n][ncol] (int64) and
 *   xhist [sampled cells][n][nbin] (each nullable, host or device).  DAZIM_E_BAD_ARG when an array is asked of a handle that is not
 *   radial.
 *   dazim_mc_radial_result, one lane per (inner cell, knot pair), every fp64 sum over the rung-0 chains in chain order, tot = N *
 *   ncold: xi_mean = S0 / tot, xi_std = sqrt(max(S1 / tot - mean^2, 0)); xi_q [3] from xhist as dazim_mc_result's q, linear inside
 *   a bin, over [lo, hi] above; xi_rhat the R-hat above from the chains' rsum[0] and rsum[1]; p_gt1 = sum ngt1 / tot; corr_vh =
 *   (S2 / tot - Ev * Eh) / (sdv * sdh) with Ev, Eh, sdv, sdh the fp64 mean and population std of the two knots from sums (NaN where
 *   a std is 0); voigt_mean = S3 / tot, voigt_std likewise from S4.  All [n][ny-2][nx-2] fp32 (xi_q [3][n][ny-2][nx-2]), each
 *   nullable, host or device, rounded once.  A cell without data: xi and V of vel0's knots, std 0, the quantiles at that xi, NaN
 *   for xi_rhat, p_gt1 and corr_vh.  Refused on a handle that is not radial and before the first recorded step.
 * dazim_mc_create: vel0 [nz][ny][nx] (the last knot; the result of cells without data), vmin, vmax [nlay][ny-2][nx-2], cobs, wdat
 *   [kmax][ny-2][nx-2] (the layout of dazim_column_lsq), step = the initial s, nadapt >= 1.  Draws the start models.  Refused
 *   (DAZIM_E_BAD_ARG): nchain outside 1..64, nlay outside 1..63, kmax outside 1..60, nbin < 2, a non-finite vmin, vmax, cobs or
 *   wdat, vmin >= vmax anywhere, step outside (0, 0.5] (the range the adaptation keeps), nadapt < 1.
 * dazim_mc_proposals: the device array [nz][ncol] fp32 the next step evaluates (owned by the handle) and ncol.
 * dazim_mc_step: one step on the curves pv [kmax][ncol] (host or device) of those proposals, from any forward model; kmax and ncol
 *   state pv's shape and must be the handle's (DAZIM_E_BAD_ARG otherwise, and for a handle of another context).
 * dazim_mc_run: nburn burn-in then nsample recorded steps, each one dazim_dispersion_kernels call (nx = ncol, ny = 1, curves only,
 *   depz [nz] and periods [kmax] host arrays as there) and one step launch; no other host wait.  n_no_root (nullable) = proposals
 *   of the run with chi2' = +inf.  Stats: "mc" (seconds of the run), "mc.disp" (its dispersion kernels), "mc.step" (its step
 *   kernels), "mc.steps", "mc.accept" (accepted / decisions of its recorded steps), "mc.no_root", "mc.proposal" (the kind) and
 *   "mc.cov_cells" (cells with cov_set = 1 at its end); "mc.ntemp", and "mc.swap_min" and "mc.swap_med", the lowest and the median
 *   of swap_acc / swap_try over the (cell, rung pair)s with a try, from all the handle's steps (0 without tempering), copied once
 *   after the run's closing wait.  With tempering "mc.accept" counts the decisions of the rung-0 chains only.
 * dazim_mc_set_proposal: kind 0 (the default) or 1; kind 1 allocates the arrays above.  DAZIM_E_BAD_ARG for another kind, for a
 *   handle of another context, or once a step has been done.
 * dazim_mc_cov_state: kind, and for kind 1 copies of cov_n, cov_set [sampled cells], cov_s1 [sampled cells][nlay], cov_s2, chol
 *   [sampled cells][npair] (each pointer nullable, host or device).  DAZIM_E_BAD_ARG for kind 0 when an array is requested.
 * dazim_mc_set_tempering: ntemp rungs up to temperature tmax, a swap round every nswap steps; ntemp = 1 restores the default (tmax
 *   is not looked at then).  It may come before or after dazim_mc_set_proposal.  DAZIM_E_BAD_ARG when ntemp is outside 1..nchain or
 *   does not divide nchain, when ntemp > 1 and tmax is not finite or <= 1, when nswap < 1, for a handle of another context, or once
 *   a step has been done.
 * dazim_mc_temper_state: ntemp, tmax, nswap, and for ntemp > 1 copies of beta [ntemp], scale [sampled cells][ntemp], swap_try and
 *   swap_acc [sampled cells][ntemp - 1] (each pointer nullable, host or device).  DAZIM_E_BAD_ARG for ntemp = 1 when an array is
 *   requested.
 * dazim_mc_state: copies of the chain state (each pointer nullable, host or device): cur [nz][ncol], chi2 [ncol], scale [sampled
 *   cells], step (steps done), sums [2][nlay][ncol], hist [sampled cells][nlay][nbin], accepted [ncol], best [nlay][sampled cells]
 *   and best_chi2 [sampled cells] (vel0's knots and +inf before the first recorded step).
 * dazim_mc_result: over the recorded steps (N of them, M = nchain): mean, std (population, of the N*M states), best, rhat [nlay][ny-2]
 *   [nx-2]; q [3][nlay][ny-2][nx-2] = 2.5 / 50 / 97.5 % of the counts, linear inside a bin; accept, chi2_best [ny-2][nx-2].  R-hat is
 *   BDA3's, chains not split: sqrt(((N-1)/N W + B/N) / W), NaN for M = 1 or N = 1.  Cells without data: mean = q = best = vel0's
 *   knots, std 0, rhat NaN, accept 0, chi2_best 0.  Refused before the first recorded step.                                      */
typedef struct dazim_mc dazim_mc;
int dazim_mc_create(dazim_ctx *ctx, int nx, int ny, int nz, int kmax, int nchain, int nbin, unsigned long long seed, const float *vel0,
                    const float *vmin, const float *vmax, const float *cobs, const float *wdat, float step, int nadapt, dazim_mc **mc,
                    int *n_empty);
int dazim_mc_proposals(dazim_mc *mc, float **vel_dev, int64_t *ncol);
int dazim_mc_set_proposal(dazim_ctx *ctx, dazim_mc *mc, int kind);
int dazim_mc_cov_state(dazim_ctx *ctx, dazim_mc *mc, int *kind, int64_t *cov_n, double *cov_s1, double *cov_s2, double *chol,
                       int *cov_set);
int dazim_mc_set_tempering(dazim_ctx *ctx, dazim_mc *mc, int ntemp, float tmax, int nswap);
int dazim_mc_temper_state(dazim_ctx *ctx, dazim_mc *mc, int *ntemp, float *tmax, int *nswap, double *beta, float *scale,
                          int64_t *swap_try, int64_t *swap_acc);
int dazim_mc_set_aniso(dazim_ctx *ctx, dazim_mc *mc, int nthin, const float *amap, const float *wa, float smooth, float damp);
int dazim_mc_aniso_step(dazim_ctx *ctx, dazim_mc *mc, int kmax, int64_t ncolc, const float *lsen);
int dazim_mc_aniso_state(dazim_ctx *ctx, dazim_mc *mc, int *nthin, double *asum, double *avar, int64_t *acnt, int64_t *skipped);
int dazim_mc_aniso_result(dazim_ctx *ctx, dazim_mc *mc, float *mean, float *std, float *std_between, float *cov_cs, int64_t *nsamp);
int dazim_mc_set_noise(dazim_ctx *ctx, dazim_mc *mc, float a0, float b0);
int dazim_mc_noise_state(dazim_ctx *ctx, dazim_mc *mc, float *a0, float *b0, double *nsum, int64_t *ncnt);
int dazim_mc_noise_result(dazim_ctx *ctx, dazim_mc *mc, float *lam_mean, float *lam_std, int *ndata);
int dazim_mc_set_noise_groups(dazim_ctx *ctx, dazim_mc *mc, int ngroup, const int *group_of_period, const float *a0, const float *b0);
int dazim_mc_noise_groups_state(dazim_ctx *ctx, dazim_mc *mc, int *ngroup, int *group_of_period, float *a0, float *b0, double *chi2g,
                                double *nsum, int64_t *ncnt);
int dazim_mc_noise_groups_result(dazim_ctx *ctx, dazim_mc *mc, float *lam_mean, float *lam_std, int *ndata);
int dazim_mc_set_segments(dazim_ctx *ctx, dazim_mc *mc, int nseg, const int *seg_iwave, const int *seg_igr, const int *seg_kmax);
int dazim_mc_set_prior(dazim_ctx *ctx, dazim_mc *mc, float smooth, float damp, const float *vref);
int dazim_mc_prior_state(dazim_ctx *ctx, dazim_mc *mc, float *smooth, float *damp, float *vref, double *q);
int dazim_mc_set_radial(dazim_ctx *ctx, dazim_mc *mc, float couple);
int dazim_mc_radial_models(dazim_mc *mc, float **vsv_dev, float **vsh_dev, int64_t *ncol);
int dazim_mc_radial_state(dazim_ctx *ctx, dazim_mc *mc, int *n, float *couple, double *rsum, int64_t *ngt1, unsigned *xhist);
int dazim_mc_radial_result(dazim_ctx *ctx, dazim_mc *mc, float *xi_mean, float *xi_std, float *xi_q, float *xi_rhat, float *p_gt1,
                           float *corr_vh, float *voigt_mean, float *voigt_std);
int dazim_mc_step(dazim_ctx *ctx, dazim_mc *mc, int kmax, int64_t ncol, const double *pv, int record);
int dazim_mc_run(dazim_ctx *ctx, dazim_mc *mc, const float *depz, float sublayers, const double *periods, int nburn, int nsample,
                 int64_t *n_no_root);
int dazim_mc_state(dazim_ctx *ctx, dazim_mc *mc, float *cur, double *chi2, float *scale, int64_t *step, double *sums, unsigned *hist,
                   int64_t *accepted, float *best, double *best_chi2);
int dazim_mc_result(dazim_ctx *ctx, dazim_mc *mc, float *mean, float *std, float *q, float *best, float *rhat, float *accept,
                    float *chi2_best);
int dazim_mc_free(dazim_ctx *ctx, dazim_mc *mc);

/* ---- N4: what surrounds the solve in the outer iteration, on the device ------------------------------
 * = TikhonovRegularization / TikhRegul_joint (inv/TikhRegul.f90:2-104, :107-209): appends nblock * maxvp rows, maxvp =
 *   (nx-2)(ny-2)(nz-1); block b regularises columns b*maxvp+1 .. (b+1)*maxvp with weight w[b] (host array): a cell on a face
 *   of the block gets the single entry 2w, an inner cell the 7-point Laplacian 6w, -w x 6.  Rows in the reference's k, j, i order. */
int dazim_csr_append_tikhonov(dazim_ctx *ctx, dazim_csr *A, int nx, int ny, int nz, int nblock, const float *w);
/* = residual cbst = obst - dsyn, CalDdatSigma (inv/CalSigamNorm.f90:2-41), datweight = 1/sigmaT, cbst *= datweight and
 *   rw(i) = rw(i)*datweight(iw(1+i)) on the first dall rows of G (inv/Main_Jt.f90:432-469).  obst, dsyn [dall] in; res
 *   (the reference's Tdata), datweight, rhs [dall] out; host or device arrays; G nullable.  stats (host, 8 floats, nullable):
 *   mean, std, mean |.|, rms of res; meandeltaT, stddeltaT; mean datweight; mean |rhs|.  The two sums of CalDdatSigma run in
 *   the reference's sequential fp32 order, so the weights are the reference's bit for bit.                              */
int dazim_weight_data(dazim_ctx *ctx, dazim_csr *G, int64_t dall, const float *obst, const float *dsyn, float *res,
                      float *datweight, float *rhs, float *stats);
/* = the clamped model update (inv/Main_Jt.f90:582-620): dv [maxvp, or 3*maxvp when joint] in/out (dVs clamped to +-0.5, zeroed
 *   below 1e-5), vs [nz][ny][nx] in/out (inner cells += dVs, clamped to [minvel, maxvel]), gc, gs [nz-1][ny-2][nx-2] out
 *   (joint; nullable).  stats (host, nullable): [nblock][nz-1][3] = min, max, sum |.| of the update per block and depth.   */
int dazim_model_update(dazim_ctx *ctx, int nx, int ny, int nz, int joint, float *vs, float *dv, float minvel, float maxvel,
                       float *gc, float *gs, float *stats);

/* = aprod (inv/aprod.f90:7): mode 1: y(m) += A*x(n) ; mode 2: x(n) += A^T*y(m)                    */
int dazim_aprod(dazim_ctx *ctx, int mode, const dazim_csr *A, float *x, float *y);

/* ---- multi-GPU solve: rows of [G; L] sharded over ranks (one process per GPU), SURVEY 8e -----------------------
 * dazim_comm_unique_id: rank 0 makes the 128-byte RCCL id and hands it to the other ranks (any transport: MPI,
 * torch.distributed, a file); dazim_comm_init: every rank joins with the same id (ncclCommInitRank on the ctx's device).
 * While a communicator is attached, dazim_lsmr treats A and b as THIS rank's row shard of one global system: per iteration
 * ONE collective on the ctx stream -- an all-gather of the n fp32 of A_p^T u_p with the double ||u_p||^2 (each rank scales its
 * shard of u by its own norm first; the sums over the ranks are formed in rank order, beta follows) --; x, v, h, hbar and the
 * reorthogonalisation window are replicated, so every rank returns the same x.  dazim_comm_free detaches.             */
int dazim_comm_unique_id(void *id128);
int dazim_comm_init(dazim_ctx *ctx, int nranks, int rank, const void *id128);
int dazim_comm_free(dazim_ctx *ctx);
/* The same communicator over FILES in a directory every rank sees (each collective staged through the host): for tests -- the
 * whole multi-rank path with two or three processes on ONE GPU, which RCCL refuses -- not for production.                      */
int dazim_comm_init_files(dazim_ctx *ctx, int nranks, int rank, const char *dir);
/* recv[r*count .. (r+1)*count) = rank r's `count` values at send, on every rank; send, recv: host or device pointers (each on its
 * own); dtype as for dazim_comm_allreduce.  No communicator attached: recv = send.  Both transports move bytes only (RCCL:
 * ncclAllGather on the ctx stream); every SUM over the ranks in this library -- dazim_comm_allreduce, the row-sharded LSMR -- is an
 * all-gather followed by one kernel that adds the ranks' values in RANK ORDER, so that RCCL and the file transport, and every rank,
 * return the same bits (SURVEY 8e "fix reduction order"; the reference's sums are sequential, inv/aprod.f90:40-55).  Option
 * "comm.allreduce" = 1: ncclAllReduce instead (RCCL's own order). */
int dazim_comm_allgather(dazim_ctx *ctx, const void *send, void *recv, int64_t count, int dtype);
/* sum (op 0) / max (op 1) over the ranks of `count` values in place; buf: host or device pointer; dtype 0 fp32, 1 fp64, 2 int64.
 * No communicator attached: nothing happens.  What a sharded host program reduces its statistics and outputs with
 * (host/dazim_main.f90, DAZIM_NGPU; the reference has no counterpart: inv/Main_Jt.f90 is one process).                         */
int dazim_comm_allreduce(dazim_ctx *ctx, void *buf, int64_t count, int dtype, int op);
/* The two N4 calls for one rank's share of a row-sharded system (host/dazim_main.f90 with DAZIM_NGPU): the regularisation rows
 * [row_lo, row_hi) of the nblock*maxvp (inv/TikhRegul.f90:2-209), and the data weights of the data rows [row0, row0 + dall) of
 * dall_glob -- meandeltaT / stddeltaT (inv/CalSigamNorm.f90:20-31) are taken over ALL data in the reference's summation order on
 * every rank, the statistics returned are the whole data set's.                                                                */
int dazim_csr_append_tikhonov_rows(dazim_ctx *ctx, dazim_csr *A, int nx, int ny, int nz, int nblock, const float *w,
                                   int64_t row_lo, int64_t row_hi);
int dazim_weight_data_sharded(dazim_ctx *ctx, dazim_csr *G, int64_t dall, int64_t row0, int64_t dall_glob, const float *obst,
                              const float *dsyn, float *res, float *wgt, float *rhs, float *stats);

/* The model's tables with the model's rows sharded over the ranks: the reference's one parallel loop (OpenMP over the columns jj,
 * inv/CalSurfG.f90:39-43 called at :1078; depthkernelTI inv/depthkernelTI.f90:2-112).  Same arguments and results as
 * dazim_dispersion_kernels / dazim_ti_kernels.  With a communicator attached, this rank computes the model rows [lo, hi) of the even
 * contiguous split of ny (columns are numbered jj*nx+ii: a block of rows is a block of columns) with the same kernels, and
 * all-gathers join the blocks: every rank returns the complete tables, bit-identical to the single-rank call.  pvRc is joined
 * before the call returns; with option "disp.async" and device-resident sen_* the perturbed copies of this rank's block run on the
 * auxiliary stream as in the single-rank call and the gather of the three depth-kernel tables follows them when that stream is
 * joined (dazim_rays_build_G*, dazim_sync, a copy that touches the tables).  Every rank must make the same calls in the same order.
 * Without a communicator: the plain calls.                                                                                     */
int dazim_dispersion_kernels_sharded(dazim_ctx *ctx, int nx, int ny, int nz, const float *vel, const float *depz, float sublayers,
                                     int kmax, const double *periods, double *pvRc, double *sen_vs, double *sen_vp,
                                     double *sen_rho, int *n_failed);
int dazim_ti_kernels_sharded(dazim_ctx *ctx, int nx, int ny, int nz, const float *vel, const float *depz, float sublayers,
                             int kmax, const double *periods, const double *pvRc, float *Lsen_Gsc);

/* = LSMR (inv/lsmrModule.f90:36), fp32 like the reference; b[m] in, x[n] out.                     */
int dazim_lsmr(dazim_ctx *ctx, const dazim_csr *A, const float *b, float damp, float atol,
               float btol, float conlim, int itnlim, int localSize, float *x, int *istop, int *itn,
               float *normA, float *condA, float *normr, float *normAr, float *normx);

/* One line of the reference's iteration log (unit nout, inv/lsmrModule.f90:667-682, format 1500:
 * itn, x(1), normr, normAr, test1, test2, normA, condA) plus test3 and rtol, which together with ctol/atol decide
 * whether the reference prints the line (:653-661).  Record 0 is the line printed before the loop (:468-471).  */
typedef struct {
  int itn;
  float x1, normr, normAr, test1, test2, test3, rtol, normA, condA;
} dazim_lsmr_rec;
/* dazim_lsmr that also returns the iteration log: trace[0..*trace_n) (HOST array of trace_cap records; iterations
 * beyond trace_cap-1 are not recorded).  The Fortran drop-in LSMR prints it to `nout` in the reference's formats.  */
int dazim_lsmr_traced(dazim_ctx *ctx, const dazim_csr *A, const float *b, float damp, float atol,
                      float btol, float conlim, int itnlim, int localSize, float *x, int *istop, int *itn,
                      float *normA, float *condA, float *normr, float *normAr, float *normx,
                      dazim_lsmr_rec *trace, int trace_cap, int *trace_n);

#ifdef __cplusplus
}
#endif
#endif
