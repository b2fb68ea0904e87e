"""dazimsurftomo_amd -- host-side mirror of the DAzimSurfTomo hot-path interface over libdazim_hip.so.

The functions keep the reference's names and argument meaning (depthkernel, gridder+travel as
`fmm_batch`, CalSurfG, aprod, LSMR; reference files cited in include/dazim.h) and call the
hand-written gfx950 kernels through the C ABI.  Arrays may be numpy arrays (staged over PCIe by the
library) or torch CUDA tensors (used in place).  Nothing here computes on the CPU: without the
built library and a GPU every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Geom, RefBox, build, load

RMAX = 129
PI_F32 = np.float32(3.1415926535898)  # inv/CalSurfG.f90:166


# status codes of include/dazim.h
DAZIM_OK, DAZIM_E_SOURCE_OUTSIDE, DAZIM_E_RECEIVER_OUTSIDE, DAZIM_E_NNZ_OVERFLOW, DAZIM_E_BAD_ARG, DAZIM_E_ROOT_NOT_FOUND = 0, 1, 2, 4, 5, 6


class DazimError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"dazim error {code}: {msg}")
        self.code = code


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ptr(x, dtype=None):
    """raw pointer of a numpy array or torch tensor (None -> NULL)"""
    if x is None:
        return None
    if _is_torch(x):
        assert x.is_contiguous()
        if dtype is not None:
            import torch
            want = {np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32,
                    np.int64: torch.int64}[dtype]
            assert x.dtype == want, (x.dtype, want)
        return C.c_void_p(x.data_ptr())
    assert isinstance(x, np.ndarray) and x.flags.c_contiguous
    if dtype is not None:
        assert x.dtype == dtype, (x.dtype, dtype)
    return C.c_void_p(x.ctypes.data)


def to_radians(lat_deg, lon_deg):
    """colatitude/longitude in fp32 radians exactly as inv/Main_Jt.f90:289-292 forms them"""
    lat = np.asarray(lat_deg, np.float32)
    lon = np.asarray(lon_deg, np.float32)
    return ((np.float32(90.0) - lat) * PI_F32 / np.float32(180.0)).astype(np.float32), \
        (lon * PI_F32 / np.float32(180.0)).astype(np.float32)


# dazim_lsmr_rec (include/dazim.h), and the byte Context.lsmr fills its trace array with before the call
LSMR_REC = np.dtype([("itn", "<i4")] + [(k, "<f4") for k in ("x1", "normr", "normAr", "test1", "test2", "test3", "rtol", "normA", "condA")])
LSMR_TRACE_FILL = 0xA5


def comm_unique_id():
    """128-byte RCCL id (rank 0 creates it and sends it to the other ranks)"""
    buf = C.create_string_buffer(128)
    if load().dazim_comm_unique_id(buf) != 0:
        raise RuntimeError("ncclGetUniqueId failed")
    return buf.raw


def geometry(nx, ny, goxd, gozd, dvxd, dvzd):
    g = Geom()
    rc = load().dazim_geometry(nx, ny, C.c_float(goxd), C.c_float(gozd), C.c_float(dvxd), C.c_float(dvzd), C.byref(g))
    if rc:
        raise DazimError(rc, "bad geometry")
    return g


def tradeoff_pick(chi2, reg2sum, gcv=None, logev=None):
    """the three picks of a trade-off sweep (dazim_tradeoff_pick, host only): dict(corner, gcv, evidence), -1 where there is none"""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    chi2, reg2sum, gcv, logev = f(chi2), f(reg2sum), f(gcv), f(logev)
    ic, ig, ie = C.c_int(-2), C.c_int(-2), C.c_int(-2)
    rc = load().dazim_tradeoff_pick(int(chi2.shape[0]), _ptr(chi2), _ptr(reg2sum), _ptr(gcv), _ptr(logev), C.byref(ic), C.byref(ig), C.byref(ie))
    if rc:
        raise DazimError(rc, "bad arguments to dazim_tradeoff_pick")
    return dict(corner=ic.value, gcv=ig.value, evidence=ie.value)


def map_tradeoff_total(mdata_p, chi2, reg2, dof=None, logev=None):
    """the criteria of the whole block-diagonal system from Context.map_tradeoff's per-period arrays (dazim_map_tradeoff_total, host
    only): dict(chi2, reg2sum, dof, gcv, logev), each [K], the sums over the periods; dof, gcv and logev None where not given"""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    mdata_p, chi2, reg2, dof, logev = np.ascontiguousarray(mdata_p, np.int64), f(chi2), f(reg2), f(dof), f(logev)
    K, kmax, nblk = reg2.shape
    new = lambda on: np.zeros(K, np.float64) if on else None
    out = dict(chi2=new(True), reg2sum=new(True), dof=new(dof is not None), gcv=new(dof is not None), logev=new(logev is not None))
    rc = load().dazim_map_tradeoff_total(K, kmax, nblk, _ptr(mdata_p, np.int64), _ptr(chi2), _ptr(reg2), _ptr(dof), _ptr(logev),
                                         *[_ptr(out[k]) for k in ("chi2", "reg2sum", "dof", "gcv", "logev")])
    if rc:
        raise DazimError(rc, "bad arguments to dazim_map_tradeoff_total")
    return out


def _tradeoff_args(m_data, b, nblk, scale, damp, dof, evidence, lead):
    """what Context.model_tradeoff and Context.map_tradeoff pass alike: (K, scale [K][nblk] fp32, damp [K] fp32, b, out) with out the
    fp64 outputs, [K] + lead (reg2 and dof: + [nblk]), None where dof or evidence is off"""
    scale = np.asarray(scale, np.float32)
    if scale.ndim == 1:
        scale = np.repeat(scale[:, None], nblk, axis=1)
    scale = np.ascontiguousarray(scale.reshape(-1, nblk))
    K = scale.shape[0]
    damp = np.ascontiguousarray(np.broadcast_to(np.asarray(damp, np.float32), (K,)))
    if not _is_torch(b):
        b = np.ascontiguousarray(b, np.float32)
    assert b.shape[0] == m_data
    new = lambda on, *tail: np.zeros((K,) + tuple(lead) + tail, np.float64) if on else None
    out = dict(chi2=new(True), reg2=new(True, nblk), xnorm2=new(True), logdet_a=new(True), logdet_p=new(evidence), dof=new(dof, nblk),
               gcv=new(dof), logev=new(evidence))
    return K, scale, damp, b, out


def _posterior_args(sel, shape):
    """what Context.map_posterior and Context.model_posterior pass alike: (new, sel, nsel, out) with new(*shape) an fp32 array where
    the outputs live (torch-cuda with a torch-cuda sel, numpy otherwise), sel as the call takes it and out the four mandatory arrays"""
    if sel is not None and _is_torch(sel):
        import torch
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=sel.device)
    else:
        new = lambda *shape: np.zeros(shape, np.float32)
        sel = None if sel is None else np.ascontiguousarray(sel, np.int32)
    return new, sel, 0 if sel is None else int(sel.shape[0]), {k: new(*shape) for k in ("std_post", "std_noise", "rdiag", "rsum")}


class Context:
    """One GPU context (`dazim_ctx`).  Raises if no GPU / no library: there is no CPU path."""

    def __init__(self, device=0):
        self.lib = load()
        self._h = C.c_void_p()
        self.device = int(device)
        rc = self.lib.dazim_create(C.byref(self._h), int(device))
        if rc:
            raise DazimError(rc, "dazim_create failed (no GPU visible?)")

    def close(self):
        if self._h:
            self.lib.dazim_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise DazimError(rc, self.lib.dazim_last_error(self._h).decode())

    def kernel_seconds(self, name):
        return self.lib.dazim_last_kernel_seconds(self._h, name.encode())

    def stat(self, name):
        """dazim_get_stat: a time or a count the last calls reported (docs/OPTIONS.md); KeyError for an unknown name"""
        v = C.c_double()
        if self.lib.dazim_get_stat(self._h, name.encode(), C.byref(v)) != 0:
            raise KeyError(name)
        return v.value

    def set_option(self, name, value):
        self._check(self.lib.dazim_set_option(self._h, name.encode(), int(value)))

    def sync(self):
        self._check(self.lib.dazim_sync(self._h))

    # ---- multi-GPU solve (RCCL inside the library) -------------------------------------------
    def comm_init(self, nranks, rank, uid):
        """join the RCCL communicator identified by `uid` (bytes from comm_unique_id() of rank 0); afterwards
        lsmr() treats its matrix and right-hand side as this rank's row shard of one global system"""
        buf = C.create_string_buffer(bytes(uid), 128)
        self._check(self.lib.dazim_comm_init(self._h, int(nranks), int(rank), buf))

    def comm_init_files(self, nranks, rank, directory):
        """the same communicator with every collective staged through files in `directory` (tests: several ranks on ONE GPU)"""
        self._check(self.lib.dazim_comm_init_files(self._h, int(nranks), int(rank), str(directory).encode()))

    def comm_allreduce(self, arr, op="sum"):
        """in-place sum / max over the ranks of a numpy array (float32, float64 or int64); nothing happens without a communicator"""
        dt = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int64): 2}[arr.dtype]
        assert arr.flags.c_contiguous
        self._check(self.lib.dazim_comm_allreduce(self._h, C.c_void_p(arr.ctypes.data), C.c_int64(arr.size), dt, 0 if op == "sum" else 1))
        return arr

    def comm_allgather(self, send, recv=None):
        """all-gather over the ranks: numpy `send` (float32, float64 or int64) -> recv[nranks, send.size]; one rank: a copy"""
        dt = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int64): 2}[send.dtype]
        nr = int(self.stat_or("comm.nranks", 1))
        if recv is None:
            recv = np.zeros((nr, send.size), send.dtype)
        assert send.flags.c_contiguous and recv.flags.c_contiguous and recv.size == nr * send.size
        self._check(self.lib.dazim_comm_allgather(self._h, C.c_void_p(send.ctypes.data), C.c_void_p(recv.ctypes.data), C.c_int64(send.size), dt))
        return recv

    def stat_or(self, name, default):
        try:
            return self.stat(name)
        except KeyError:
            return default

    def comm_free(self):
        self._check(self.lib.dazim_comm_free(self._h))

    # ---- K1 ---------------------------------------------------------------------------------
    def depthkernel(self, vel, depz, tRc, minthk, kernels=True, pv=None, sen=None, sharded=False):
        """depthkernel (inv/CalSurfG.f90:1): vel[nz][ny][nx] -> pvRc[kmax][nx*ny] and, if `kernels`,
        (sen_vs, sen_vp, sen_rho)[nz][kmax][nx*ny].  Returns (pv, sen, n_failed).
        sharded: dazim_dispersion_kernels_sharded -- with a communicator attached this rank computes its block of the model's
        rows and all-gathers join the tables (every rank must call)."""
        nz, ny, nx = vel.shape
        depz = np.ascontiguousarray(depz, np.float32)
        tRc = np.ascontiguousarray(tRc, np.float64)
        kmax = len(tRc)
        if _is_torch(vel):
            import torch
            if pv is None:
                pv = torch.empty((kmax, nx * ny), dtype=torch.float64, device=vel.device)
            if kernels and sen is None:
                sen = [torch.empty((nz, kmax, nx * ny), dtype=torch.float64, device=vel.device) for _ in range(3)]
        else:
            vel = np.ascontiguousarray(vel, np.float32)
            if pv is None:
                pv = np.zeros((kmax, nx * ny), np.float64)
            if kernels and sen is None:
                sen = [np.zeros((nz, kmax, nx * ny), np.float64) for _ in range(3)]
        nf = C.c_int(0)
        sp = [_ptr(a) for a in sen] if kernels else [None] * 3
        fn = self.lib.dazim_dispersion_kernels_sharded if sharded else self.lib.dazim_dispersion_kernels
        rc = fn(self._h, nx, ny, nz, _ptr(vel, np.float32), _ptr(depz), C.c_float(minthk),
                kmax, _ptr(tRc), _ptr(pv), sp[0], sp[1], sp[2], C.byref(nf))
        self._check(rc)
        return pv, (sen if kernels else None), nf.value

    def dispersion_kernels_typed(self, vel, depz, segments, sublayers, kernels=True):
        """dazim_dispersion_kernels_typed: depthkernel for every wave type.  segments = [(iwave, igr, periods), ...] with iwave 1 Love /
        2 Rayleigh and igr 0 phase / 1 group velocity; the tables are indexed by the K virtual periods, the segments' periods laid
        end to end.  vel[nz][ny][nx] -> pv[K][nx*ny] and, if `kernels`, (sen_vs, sen_vp, sen_rho)[nz][K][nx*ny].
        Returns (pv, sen, n_failed)."""
        nz, ny, nx = vel.shape
        depz = np.ascontiguousarray(depz, np.float32)
        iw = np.ascontiguousarray([s[0] for s in segments], np.int32)
        ig = np.ascontiguousarray([s[1] for s in segments], np.int32)
        km = np.ascontiguousarray([len(s[2]) for s in segments], np.int32)
        t = np.ascontiguousarray(np.concatenate([np.asarray(s[2], np.float64).ravel() for s in segments]) if len(segments) else np.zeros(0))
        K = len(t)
        if _is_torch(vel):
            import torch
            pv = torch.empty((K, nx * ny), dtype=torch.float64, device=vel.device)
            sen = [torch.empty((nz, K, nx * ny), dtype=torch.float64, device=vel.device) for _ in range(3)] if kernels else None
        else:
            vel = np.ascontiguousarray(vel, np.float32)
            pv = np.zeros((K, nx * ny), np.float64)
            sen = [np.zeros((nz, K, nx * ny), np.float64) for _ in range(3)] if kernels else None
        nf = C.c_int(0)
        sp = [_ptr(a) for a in sen] if kernels else [None] * 3
        rc = self.lib.dazim_dispersion_kernels_typed(self._h, nx, ny, nz, _ptr(vel, np.float32), _ptr(depz), C.c_float(sublayers), len(segments),
                                                     _ptr(iw), _ptr(ig), _ptr(km), _ptr(t), _ptr(pv), sp[0], sp[1], sp[2], C.byref(nf))
        self._check(rc)
        return pv, sen, nf.value

    def surfdisp96(self, thk, vp, vs, rho, t, iflsph=1, iwave=2, mode=1, igr=0, nlayer=None):
        """surfdisp96 (inv/surfdisp96.f:52) with the subroutine's own arguments, for one model (1-D arrays) or a batch
        (thk, vp, vs, rho [nmodel][nlayer_max], `nlayer` [nmodel] if the models have different numbers of layers):
        iwave 1 Love / 2 Rayleigh, mode 1 = fundamental, igr 0 phase / 1 group velocity, iflsph 0 flat / 1 spherical.
        Returns (cg [nmodel][kmax] or [kmax], n_failed)."""
        a = [np.ascontiguousarray(x, np.float32) for x in (thk, vp, vs, rho)]
        single = a[0].ndim == 1
        if single:
            a = [x[None, :] for x in a]
        nmodel, nlm = a[0].shape
        nl = np.full(nmodel, nlm, np.int32) if nlayer is None else np.ascontiguousarray(nlayer, np.int32)
        t = np.ascontiguousarray(t, np.float64)
        cg = np.zeros((nmodel, len(t)), np.float64)
        nf = C.c_int(0)
        rc = self.lib.dazim_surfdisp96(self._h, nmodel, nlm, _ptr(nl), _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]),
                                       int(iflsph), int(iwave), int(mode), int(igr), len(t), _ptr(t), _ptr(cg), C.byref(nf))
        self._check(rc)
        return (cg[0] if single else cg), nf.value

    # ---- N1 --------------------------------------------------------------------------------
    def ti_kernels(self, vel, depz, tRc, minthk, pv, lsen=None, sharded=False):
        """depthkernelTI/tregn96 (inv/depthkernelTI.f90:2): vel[nz][ny][nx] and pvRc[kmax][nx*ny] (output of
        depthkernel) -> Lsen_Gsc[nz-1][kmax][nx*ny] fp32.  sharded: dazim_ti_kernels_sharded (see depthkernel)."""
        nz, ny, nx = vel.shape
        depz = np.ascontiguousarray(depz, np.float32)
        tRc = np.ascontiguousarray(tRc, np.float64)
        kmax = len(tRc)
        if _is_torch(vel):
            import torch
            if lsen is None:
                lsen = torch.empty((nz - 1, kmax, nx * ny), dtype=torch.float32, device=vel.device)
        else:
            vel = np.ascontiguousarray(vel, np.float32)
            pv = np.ascontiguousarray(pv, np.float64)
            if lsen is None:
                lsen = np.zeros((nz - 1, kmax, nx * ny), np.float32)
        fn = self.lib.dazim_ti_kernels_sharded if sharded else self.lib.dazim_ti_kernels
        rc = fn(self._h, nx, ny, nz, _ptr(vel, np.float32), _ptr(depz), C.c_float(minthk), kmax, _ptr(tRc), _ptr(pv), _ptr(lsen))
        self._check(rc)
        return lsen

    # ---- K2+K3 -----------------------------------------------------------------------------
    def fmm_batch(self, nx, ny, goxd, gozd, dvxd, dvzd, pv, scx, scz, period_idx,
                  veln=None, ttn=None, ttnr=None, nstsr=None, boxes=None, status=None,
                  want_refined=True, keep_fields=False):
        """gridder + bsplrefine + travel x2 for a batch of (source, period) fields
        (body of the source loop inv/CalSurfG.f90:1146-1314).  Returns a dict of outputs; numpy
        in -> numpy out, torch-cuda in -> the given output tensors are filled in place.
        keep_fields: ttn = NULL -- the coarse fields stay inside the library (in the eikonal kernel's tiles) for the
        rays_build_G call that follows, as in the reference's CalSurfG, which never returns them (out["ttn"] is None)."""
        g = geometry(nx, ny, goxd, gozd, dvxd, dvzd)
        kmax = pv.shape[0]
        nfield = int(scx.shape[0])
        if not _is_torch(pv):
            pv = np.ascontiguousarray(pv, np.float64)
            scx = np.ascontiguousarray(scx, np.float32)
            scz = np.ascontiguousarray(scz, np.float32)
            period_idx = np.ascontiguousarray(period_idx, np.int32)
            if ttn is None and not keep_fields:
                ttn = np.zeros((nfield, g.nnx, g.nnz), np.float32)
            if veln is None:
                veln = np.zeros((kmax, g.nnx, g.nnz), np.float32)
            if want_refined and ttnr is None:
                ttnr = np.zeros((nfield, RMAX, RMAX), np.float32)
                nstsr = np.zeros((nfield, RMAX, RMAX), np.int32)
            if boxes is None:
                boxes = (RefBox * max(nfield, 1))()
            if status is None:
                status = np.zeros(nfield, np.int32)
        if keep_fields:
            ttn = None
        bptr = None
        if boxes is not None:
            bptr = C.c_void_p(boxes.data_ptr()) if _is_torch(boxes) else C.cast(boxes, C.c_void_p)
        rc = self.lib.dazim_fmm_batch(self._h, nx, ny, C.c_float(goxd), C.c_float(gozd), C.c_float(dvxd),
                                      C.c_float(dvzd), kmax, _ptr(pv), nfield, _ptr(scx), _ptr(scz),
                                      _ptr(period_idx), _ptr(veln), _ptr(ttn), _ptr(ttnr), _ptr(nstsr),
                                      bptr, _ptr(status))
        out = dict(geom=g, veln=veln, ttn=ttn, ttnr=ttnr, nstsr=nstsr, boxes=boxes, status=status, rc=rc)
        if rc:
            err = DazimError(rc, self.lib.dazim_last_error(self._h).decode())
            err.partial = out
            raise err
        return out

    # ---- K4+K5 -------------------------------------------------------------------------------
    def _check_rays(self, rc, tpred, nnz, nb):
        """a ray call that failed on a ray's status (receiver outside) has still filled in the other rays' times, the entry count of
        their rows and the boundary count: the error carries them as `partial` (there is no matrix)"""
        if rc:
            err = DazimError(rc, self.lib.dazim_last_error(self._h).decode())
            err.partial = {"tpred": tpred, "nnz": nnz.value, "n_boundary": nb.value}
            raise err

    def rays_build_G(self, nx, ny, goxd, gozd, dvxd, dvzd, vels, fields, scx, scz, period_idx, field_of_ray,
                     rcx, rcz, sen, kernel_idx=None, tpred=None, lsen=None):
        """srtimes + rpaths + row assembly (receiver loop of CalSurfG, inv/CalSurfG.f90:1326-1364).
        `fields` is the dict returned by fmm_batch for the same scx/scz/period_idx.
        Returns (G, tpred, n_boundary)."""
        nz = vels.shape[0]
        kmax = fields["veln"].shape[0]
        nfield = int(scx.shape[0])
        nray = int(rcx.shape[0])
        if tpred is None:
            if _is_torch(rcx):
                import torch
                tpred = torch.empty(nray, dtype=torch.float32, device=rcx.device)
            else:
                tpred = np.zeros(nray, np.float32)
        boxes = fields["boxes"]
        bptr = C.c_void_p(boxes.data_ptr()) if _is_torch(boxes) else C.cast(boxes, C.c_void_p)
        h = C.c_void_p()
        nnz = C.c_int64(0)
        nb = C.c_int(0)
        args = [self._h, nx, ny, nz, C.c_float(goxd), C.c_float(gozd), C.c_float(dvxd),
                C.c_float(dvzd), kmax, _ptr(vels, np.float32), nfield, _ptr(scx), _ptr(scz),
                _ptr(period_idx), _ptr(kernel_idx), _ptr(fields["veln"]), _ptr(fields["ttn"]),
                _ptr(fields["ttnr"]), _ptr(fields["nstsr"]), bptr, C.c_int64(nray),
                _ptr(field_of_ray), _ptr(rcx), _ptr(rcz), _ptr(sen[0]), _ptr(sen[1]), _ptr(sen[2])]
        tail = [_ptr(tpred), C.byref(h), C.byref(nnz), C.byref(nb)]
        if lsen is None:   # isotropic rows (CalSurfG)
            rc = self.lib.dazim_rays_build_G(*args, *tail)
        else:              # joint rows dVs | Gc | Gs (CalSurfGAnisoJoint), lsen = Lsen_Gsc[nz-1][kmax][nx*ny]
            rc = self.lib.dazim_rays_build_G_joint(*args, _ptr(lsen, np.float32), *tail)
        self._check_rays(rc, tpred, nnz, nb)
        n = (nx - 2) * (ny - 2) * (nz - 1) * (1 if lsen is None else 3)
        return SparseMatrix(self, h, nray, n, nnz.value), tpred, nb.value

    def rays_build_G_maps(self, nx, ny, goxd, gozd, dvxd, dvzd, fields, scx, scz, period_idx, field_of_ray, rcx, rcz,
                          azim=False, tpred=None):
        """map rows of the per-period phase-velocity (and, with `azim`, 2-psi a1/a2) inversion: the rows of rays_build_G / the
        joint mode with unit depth kernels and nz = 2, the Frechet values fdm (, fdmc, fdms) themselves, one column block per period
        (column blk*kmax*ncell + (period_idx-1)*ncell + (jj-1)*nvx + kk-1).  Returns (G, tpred, n_boundary)."""
        kmax = fields["veln"].shape[0]
        nfield = int(scx.shape[0])
        nray = int(rcx.shape[0])
        if tpred is None:
            if _is_torch(rcx):
                import torch
                tpred = torch.empty(nray, dtype=torch.float32, device=rcx.device)
            else:
                tpred = np.zeros(nray, np.float32)
        boxes = fields["boxes"]
        bptr = C.c_void_p(boxes.data_ptr()) if _is_torch(boxes) else C.cast(boxes, C.c_void_p)
        h = C.c_void_p()
        nnz = C.c_int64(0)
        nb = C.c_int(0)
        rc = self.lib.dazim_rays_build_G_maps(self._h, nx, ny, C.c_float(goxd), C.c_float(gozd), C.c_float(dvxd), C.c_float(dvzd),
                                              kmax, int(bool(azim)), nfield, _ptr(scx), _ptr(scz), _ptr(period_idx),
                                              _ptr(fields["veln"]), _ptr(fields["ttn"]), _ptr(fields["ttnr"]), _ptr(fields["nstsr"]),
                                              bptr, C.c_int64(nray), _ptr(field_of_ray), _ptr(rcx), _ptr(rcz), _ptr(tpred),
                                              C.byref(h), C.byref(nnz), C.byref(nb))
        self._check_rays(rc, tpred, nnz, nb)
        n = (nx - 2) * (ny - 2) * kmax * (3 if azim else 1)
        return SparseMatrix(self, h, nray, n, nnz.value), tpred, nb.value

    def phase_map_update(self, nx, ny, pv, dm, minc, maxc, azim):
        """clamped update of the per-period maps (dazim_phase_map_update): pv[kmax][ny*nx] fp64 (the fmm_batch maps) and dm (c | a1 |
        a2 blocks) are updated in place (numpy).  Returns (a1, a2, stats[nblock][kmax][3]); a1, a2 [kmax][ny-2][nx-2] or None."""
        kmax = pv.shape[0]
        assert pv.size == kmax * nx * ny and pv.flags.c_contiguous
        ncell = (nx - 2) * (ny - 2)
        nblock = 3 if azim else 1
        assert pv.dtype == np.float64 and dm.dtype == np.float32 and len(dm) == ncell * kmax * nblock
        a1 = np.zeros((kmax, ny - 2, nx - 2), np.float32) if azim else None
        a2 = np.zeros((kmax, ny - 2, nx - 2), np.float32) if azim else None
        st = np.zeros((nblock, kmax, 3), np.float32)
        self._check(self.lib.dazim_phase_map_update(self._h, nx, ny, kmax, int(bool(azim)), _ptr(pv), _ptr(dm), C.c_float(minc),
                                                    C.c_float(maxc), _ptr(a1), _ptr(a2), _ptr(st)))
        return a1, a2, st

    def vs_kernels(self, vel, sen, skern=None):
        """dc/dVs table of the 3-D rows (dazim_vs_kernels): vel[nz][ny][nx] and sen = (sen_vs, sen_vp, sen_rho) from depthkernel ->
        skern[nz][kmax][nx*ny] fp64, the table dazim_rays_build_G multiplies.  numpy in -> numpy out; torch-cuda in -> filled in place."""
        nz, ny, nx = vel.shape
        kmax = sen[0].shape[1]
        if skern is None:
            if _is_torch(vel):
                import torch
                skern = torch.empty((nz, kmax, nx * ny), dtype=torch.float64, device=vel.device)
            else:
                skern = np.zeros((nz, kmax, nx * ny), np.float64)
        if not _is_torch(vel):
            vel = np.ascontiguousarray(vel, np.float32)
            sen = [np.ascontiguousarray(s, np.float64) for s in sen]
        self._check(self.lib.dazim_vs_kernels(self._h, nx, ny, nz, kmax, _ptr(vel, np.float32), _ptr(sen[0], np.float64),
                                              _ptr(sen[1], np.float64), _ptr(sen[2], np.float64), _ptr(skern, np.float64)))
        return skern

    def column_lsq(self, nx, ny, nlay, kern, rhs, wdat=None, smooth=0.0, damp=0.0, x=None):
        """one regularised least-squares problem per inner cell (dazim_column_lsq): kern[>=nlay][kmax][nx*ny] (fp64 skern or fp32
        Lsen_Gsc), rhs[nrhs][kmax][ny-2][nx-2], wdat[kmax][ny-2][nx-2] or None (all ones).
        Returns (x[nrhs][nlay][ny-2][nx-2] fp32, n_empty, stats[nrhs][kmax][2] = RMS of r and of r - K x)."""
        kmax = kern.shape[1]
        nrhs = rhs.shape[0]
        fp32 = str(kern.dtype).endswith("float32")
        if x is None:
            if _is_torch(rhs):
                import torch
                x = torch.empty((nrhs, nlay, ny - 2, nx - 2), dtype=torch.float32, device=rhs.device)
            else:
                x = np.zeros((nrhs, nlay, ny - 2, nx - 2), np.float32)
        if not _is_torch(rhs):
            kern = np.ascontiguousarray(kern)
            rhs = np.ascontiguousarray(rhs, np.float32)
            wdat = None if wdat is None else np.ascontiguousarray(wdat, np.float32)
        ne = C.c_int(0)
        st = np.zeros((nrhs, kmax, 2), np.float32)
        self._check(self.lib.dazim_column_lsq(self._h, nx, ny, int(nlay), kmax, int(fp32), _ptr(kern, np.float32 if fp32 else np.float64),
                                              nrhs, _ptr(rhs, np.float32), _ptr(wdat, np.float32), C.c_float(smooth), C.c_float(damp),
                                              _ptr(x, np.float32), C.byref(ne), _ptr(st)))
        return x, ne.value, st

    def column_resolution(self, nx, ny, nlay, kern, wdat=None, smooth=0.0, damp=0.0, depz=None, rows=False):
        """posterior std and resolution of column_lsq's problem per inner cell and knot (dazim_column_resolution): kern, wdat, smooth,
        damp as in column_lsq, depz[nlay] the knots' depths (for `width`), rows=True for the full averaging kernels.  numpy in -> numpy
        out, torch-cuda kern -> torch-cuda arrays.  Returns a dict: std_post, std_noise, rdiag, rsum, width (None without depz), each
        [nlay][ny-2][nx-2]; rows [nlay][nlay][ny-2][nx-2] (None unless asked); trace [ny-2][nx-2]; n_empty, n_failed."""
        kmax = kern.shape[1]
        fp32 = str(kern.dtype).endswith("float32")
        if _is_torch(kern):
            import torch
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=kern.device)
        else:
            new = lambda *shape: np.zeros(shape, np.float32)
            kern = np.ascontiguousarray(kern)
            wdat = None if wdat is None else np.ascontiguousarray(wdat, np.float32)
        if depz is not None and not _is_torch(depz):
            depz = np.ascontiguousarray(depz, np.float32)
            assert depz.size == nlay
        out = {k: new(nlay, ny - 2, nx - 2) for k in ("std_post", "std_noise", "rdiag", "rsum")}
        out["width"] = None if depz is None else new(nlay, ny - 2, nx - 2)
        out["rows"] = new(nlay, nlay, ny - 2, nx - 2) if rows else None
        out["trace"] = new(ny - 2, nx - 2)
        ne, nf = C.c_int(0), C.c_int(0)
        self._check(self.lib.dazim_column_resolution(self._h, nx, ny, int(nlay), kmax, int(fp32), _ptr(kern, np.float32 if fp32 else np.float64),
                                                     _ptr(wdat, np.float32), C.c_float(smooth), C.c_float(damp), _ptr(depz, np.float32),
                                                     *[_ptr(out[k], np.float32) for k in ("std_post", "std_noise", "rdiag", "rsum", "width",
                                                                                          "rows", "trace")], C.byref(ne), C.byref(nf)))
        out["n_empty"], out["n_failed"] = ne.value, nf.value
        return out

    @staticmethod
    def _radial_args(nlay, kern_v, kern_h, *f32):
        """what column_lsq_radial and column_resolution_radial pass alike: (kv, kh, whether the arrays are torch-cuda, kern_v, kern_h, the fp32 arrays), NumPy
        arrays made contiguous; a kernel table that is None or has no period counts as absent"""
        absent = lambda k: k is None or k.shape[1] == 0
        kern_v, kern_h = (None if absent(k) else k for k in (kern_v, kern_h))
        on_dev = any(a is not None and _is_torch(a) for a in (kern_v, kern_h))
        if not on_dev:
            kern_v, kern_h = (None if k is None else np.ascontiguousarray(k, np.float64) for k in (kern_v, kern_h))
            f32 = [None if a is None else np.ascontiguousarray(a, np.float32) for a in f32]
        for k in (kern_v, kern_h):
            assert k is None or k.shape[0] >= nlay
        return (0 if kern_v is None else kern_v.shape[1], 0 if kern_h is None else kern_h.shape[1], on_dev, kern_v, kern_h, *f32)

    def column_lsq_radial(self, nx, ny, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v=None, w_h=None, d0=None, smooth=0.0, damp=0.0,
                          couple=0.0):
        """Vsv and Vsh updates per inner cell, tied by a prior towards isotropy (dazim_column_lsq_radial): kern_v[>=nlay][kv][nx*ny]
        over the Rayleigh periods, kern_h[>=nlay][kh][nx*ny] over the Love periods (fp64; None for a wave type without periods),
        rhs_* and w_*[kv|kh][ny-2][nx-2] (w None: all ones), d0[nlay][ny-2][nx-2] the current Vsh - Vsv (None: 0).
        Returns (x[2][nlay][ny-2][nx-2] fp32 = dVsv, dVsh, n_empty, stats[kv+kh][2], the Rayleigh periods first)."""
        kv, kh, on_dev, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = self._radial_args(nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0)
        if on_dev:
            import torch
            x = torch.empty((2, nlay, ny - 2, nx - 2), dtype=torch.float32, device=(kern_v if kv else kern_h).device)
        else:
            x = np.zeros((2, nlay, ny - 2, nx - 2), np.float32)
        ne = C.c_int(0)
        st = np.zeros((kv + kh, 2), np.float32)
        f32 = lambda a: _ptr(a, np.float32)
        self._check(self.lib.dazim_column_lsq_radial(self._h, nx, ny, int(nlay), kv, _ptr(kern_v, np.float64), kh, _ptr(kern_h, np.float64),
                                                     f32(rhs_v if kv else None), f32(rhs_h if kh else None), f32(w_v if kv else None),
                                                     f32(w_h if kh else None), f32(d0), C.c_float(smooth), C.c_float(damp),
                                                     C.c_float(couple), f32(x), C.byref(ne), _ptr(st)))
        return x, ne.value, st

    def column_resolution_radial(self, nx, ny, nlay, kern_v, kern_h, w_v=None, w_h=None, smooth=0.0, damp=0.0, couple=0.0, rows=False):
        """posterior std, Vsv-Vsh covariance and resolution of column_lsq_radial's problem per inner cell and knot
        (dazim_column_resolution_radial), arguments as there.  numpy in -> numpy out, torch-cuda kernels -> torch-cuda arrays.
        Returns a dict: std, rdiag, rsum, cross [2][nlay][ny-2][nx-2] (Vsv, then Vsh); cov_vh [nlay][ny-2][nx-2]; trace
        [2][ny-2][nx-2]; rows [2 nlay][2 nlay][ny-2][nx-2] (None unless asked); n_empty, n_failed."""
        kv, kh, on_dev, kern_v, kern_h, w_v, w_h = self._radial_args(nlay, kern_v, kern_h, w_v, w_h)
        if on_dev:
            import torch
            dev = (kern_v if kv else kern_h).device
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        else:
            new = lambda *shape: np.zeros(shape, np.float32)
        out = {k: new(2, nlay, ny - 2, nx - 2) for k in ("std", "rdiag", "rsum", "cross")}
        out["cov_vh"] = new(nlay, ny - 2, nx - 2)
        out["trace"] = new(2, ny - 2, nx - 2)
        out["rows"] = new(2 * nlay, 2 * nlay, ny - 2, nx - 2) if rows else None
        ne, nf = C.c_int(0), C.c_int(0)
        f32 = lambda a: _ptr(a, np.float32)
        self._check(self.lib.dazim_column_resolution_radial(self._h, nx, ny, int(nlay), kv, _ptr(kern_v, np.float64), kh,
                                                            _ptr(kern_h, np.float64), f32(w_v if kv else None), f32(w_h if kh else None),
                                                            C.c_float(smooth), C.c_float(damp), C.c_float(couple),
                                                            *[f32(out[k]) for k in ("std", "cov_vh", "rdiag", "rsum", "cross", "trace", "rows")],
                                                            C.byref(ne), C.byref(nf)))
        out["n_empty"], out["n_failed"] = ne.value, nf.value
        return out

    def map_posterior(self, A, m_data, nx, ny, kmax, azim, damp, sel=None, width=True):
        """posterior std and resolution of the per-period maps (dazim_map_posterior) from the matrix lsmr is given: A a SparseMatrix
        whose first m_data rows are the weighted data rows, damp lsmr's damping, sel local indices blk*ncell + cell whose rows of
        Rm are wanted (numpy, or torch-cuda for torch-cuda outputs).  Returns a dict: std_post, std_noise, rdiag, rsum, width (None
        when off), leak (None unless azim), each [nblk][kmax][ny-2][nx-2]; trace [nblk][kmax]; rows [kmax][nsel][n_g] (None without
        sel); n_failed."""
        nblk = 3 if azim else 1
        ng = nblk * (nx - 2) * (ny - 2)
        new, sel, nsel, out = _posterior_args(sel, (nblk, kmax, ny - 2, nx - 2))
        out["width"] = new(nblk, kmax, ny - 2, nx - 2) if width else None
        out["leak"] = new(nblk, kmax, ny - 2, nx - 2) if azim else None
        out["rows"] = new(kmax, nsel, ng) if nsel else None
        out["trace"] = new(nblk, kmax)
        nf = C.c_int(0)
        f32 = lambda k: _ptr(out[k], np.float32)
        self._check(self.lib.dazim_map_posterior(self._h, A._h, C.c_int64(int(m_data)), nx, ny, int(kmax), int(bool(azim)), C.c_float(damp),
                                                 f32("std_post"), f32("std_noise"), f32("rdiag"), f32("rsum"), f32("width"), f32("leak"),
                                                 nsel, _ptr(sel, np.int32), f32("rows"), f32("trace"), C.byref(nf)))
        out["n_failed"] = nf.value
        return out

    def map_tradeoff(self, A, m_data, b, nx, ny, kmax, azim, scale, damp, dof=True, evidence=True, x=False):
        """the maps' linearised step solved exactly at K regularisation strengths, per period (dazim_map_tradeoff, DESIGN.md section
        12.2): A, m_data as in map_posterior, b[m_data] the weighted right-hand side lsmr is given (numpy or torch-cuda), scale
        [K][nblk] (or [K]: the same factor on every block) the factors on the stored regularisation rows, damp [K] (or one value).
        Returns a dict of numpy arrays: mdata_p [kmax] int64; chi2, xnorm2, logdet_a [K][kmax] fp64; reg2 [K][kmax][nblk]; dof
        [K][kmax][nblk] and gcv [K][kmax] (None unless dof); logdet_p and logev [K][kmax] (None unless evidence); x
        [K][nblk][kmax][ny-2][nx-2] fp32 (None unless asked); n_failed [K][kmax] int32; total = dict(chi2, reg2sum, dof, gcv, logev),
        each [K], the sums over the periods (dazim_map_tradeoff_total); pick = per period dict(corner, gcv, evidence), the indices
        dazim_tradeoff_pick names (-1: none); pick_total the same from the totals."""
        nblk = 3 if azim else 1
        K, scale, damp, b, out = _tradeoff_args(m_data, b, nblk, scale, damp, dof, evidence, (kmax,))
        out["mdata_p"] = np.zeros(kmax, np.int64)
        out["x"] = np.zeros((K, nblk, kmax, ny - 2, nx - 2), np.float32) if x else None
        nf = np.zeros((K, kmax), np.int32)
        f64 = lambda k: _ptr(out[k], np.float64)
        self._check(self.lib.dazim_map_tradeoff(self._h, A._h, C.c_int64(int(m_data)), _ptr(b, np.float32), nx, ny, int(kmax), int(bool(azim)), K,
                                                _ptr(scale, np.float32), _ptr(damp, np.float32), int(bool(dof)), int(bool(evidence)),
                                                _ptr(out["mdata_p"], np.int64), f64("chi2"), f64("reg2"), f64("xnorm2"), f64("logdet_a"),
                                                f64("logdet_p"), f64("dof"), f64("gcv"), f64("logev"), _ptr(out["x"], np.float32),
                                                _ptr(nf, np.int32)))
        out["n_failed"] = nf
        out["total"] = map_tradeoff_total(out["mdata_p"], out["chi2"], out["reg2"], out["dof"], out["logev"])
        reg2sum = out["reg2"].sum(axis=2)
        col = lambda a, p: None if a is None else a[:, p]
        out["pick"] = [tradeoff_pick(out["chi2"][:, p], reg2sum[:, p], col(out["gcv"], p), col(out["logev"], p)) for p in range(kmax)]
        tot = out["total"]
        out["pick_total"] = tradeoff_pick(tot["chi2"], tot["reg2sum"], tot["gcv"], tot["logev"])
        return out

    def model_posterior(self, A, m_data, nx, ny, nz, joint, damp, depz=None, sel=None, width=True):
        """posterior std and resolution of the direct 3-D inversion (dazim_model_posterior) from the matrix lsmr is given in an outer
        iteration: A a SparseMatrix whose first m_data rows are the weighted data rows, damp lsmr's damping, depz[nz-1] the knots'
        depths (for width_z), sel indices blk*maxvp + k*ncell + cell whose rows of Rm are wanted (numpy, or torch-cuda for torch-cuda
        outputs).  Returns a dict: std_post, std_noise, rdiag, rsum, width_h (None when off), width_z (None when off or without
        depz), leak (None unless joint), each [nblk][nz-1][ny-2][nx-2]; trace [nblk][nz-1]; rows [nsel][n] (None without sel);
        n_failed."""
        nblk = 3 if joint else 1
        n = nblk * (nx - 2) * (ny - 2) * (nz - 1)
        shape = (nblk, nz - 1, ny - 2, nx - 2)
        new, sel, nsel, out = _posterior_args(sel, shape)
        if depz is not None and not _is_torch(depz):
            depz = np.ascontiguousarray(depz, np.float32)
            assert depz.size == nz - 1
        out["width_h"] = new(*shape) if width else None
        out["width_z"] = new(*shape) if width and depz is not None else None
        out["leak"] = new(*shape) if joint else None
        out["rows"] = new(nsel, n) if nsel else None
        out["trace"] = new(nblk, nz - 1)
        nf = C.c_int(0)
        f32 = lambda k: _ptr(out[k], np.float32)
        self._check(self.lib.dazim_model_posterior(self._h, A._h, C.c_int64(int(m_data)), nx, ny, nz, int(bool(joint)), C.c_float(damp),
                                                   _ptr(depz, np.float32) if out["width_z"] is not None else None, f32("std_post"),
                                                   f32("std_noise"), f32("rdiag"), f32("rsum"), f32("width_h"), f32("width_z"),
                                                   f32("leak"), nsel, _ptr(sel, np.int32), f32("rows"), f32("trace"), C.byref(nf)))
        out["n_failed"] = nf.value
        return out

    def model_tradeoff(self, A, m_data, b, nx, ny, nz, joint, scale, damp, dof=True, evidence=True, x=False):
        """the linearised step of the direct 3-D inversion solved exactly at K regularisation strengths (dazim_model_tradeoff, DESIGN.md
        section 16): A, m_data as in model_posterior, b[m_data] the weighted right-hand side lsmr is given (numpy or torch-cuda),
        scale [K][nblk] (or [K]: the same factor on every block) the factors on the stored regularisation rows, damp [K] (or one
        value).  Returns a dict of numpy fp64 arrays: chi2, xnorm2, logdet_a [K]; reg2 [K][nblk]; dof [K][nblk] and gcv [K] (None
        unless dof); logdet_p and logev [K] (None unless evidence); x [K][nblk][nz-1][ny-2][nx-2] fp32 (None unless asked); n_failed
        [K] int32; pick = dict(corner, gcv, evidence), the indices dazim_tradeoff_pick names (-1: none)."""
        nblk = 3 if joint else 1
        K, scale, damp, b, out = _tradeoff_args(m_data, b, nblk, scale, damp, dof, evidence, ())
        out["x"] = np.zeros((K, nblk, nz - 1, ny - 2, nx - 2), np.float32) if x else None
        nf = np.zeros(K, np.int32)
        f64 = lambda k: _ptr(out[k], np.float64)
        self._check(self.lib.dazim_model_tradeoff(self._h, A._h, C.c_int64(int(m_data)), _ptr(b, np.float32), nx, ny, nz, int(bool(joint)), K,
                                                  _ptr(scale, np.float32), _ptr(damp, np.float32), int(bool(dof)), int(bool(evidence)),
                                                  f64("chi2"), f64("reg2"), f64("xnorm2"), f64("logdet_a"), f64("logdet_p"), f64("dof"),
                                                  f64("gcv"), f64("logev"), _ptr(out["x"], np.float32), _ptr(nf, np.int32)))
        out["n_failed"] = nf
        out["pick"] = tradeoff_pick(out["chi2"], out["reg2"].sum(axis=1), out["gcv"], out["logev"])
        return out

    def mc_create(self, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, step=0.05, nadapt=50, proposal=0,
                  ntemp=1, tmax=1.0, nswap=1, aniso=None, noise=None, prior=None, segments=None, noise_groups=None, radial=None):
        """Monte-Carlo Vs per inner cell (dazim_mc_create): vel0[nz][ny][nx], vmin, vmax[nz-1][ny-2][nx-2],
        cobs, wdat[kmax][ny-2][nx-2].  Returns a MonteCarlo handle (draws the start models); its n_empty counts the cells without
        data.  proposal: 0 isotropic in box units, 1 shaped by the chains' covariance (MonteCarlo.set_proposal).  ntemp > 1: parallel
        tempering with ntemp rungs up to temperature tmax and a swap round every nswap steps (MonteCarlo.set_tempering).  aniso: a
        dict of MonteCarlo.set_aniso's arguments (nthin, amap, wa, smooth, damp) switches the Gc/Gs posteriors on.  noise: (a0, b0)
        makes the data-noise scale of every cell an unknown with the prior lambda^2 ~ InverseGamma(a0, b0) (MonteCarlo.set_noise).
        prior: (smooth, damp) or (smooth, damp, vref) adds the Gaussian smoothness prior to the box (MonteCarlo.set_prior).
        segments: [(iwave, igr, periods), ...] makes the kmax periods those of several wave types (MonteCarlo.set_segments).
        noise_groups: (group_of_period, a0, b0) gives every group of periods a noise scale of its own (MonteCarlo.set_noise_groups).
        radial: couple makes the knots the stacked [Vsv, Vsh, deepest] of radial anisotropy (MonteCarlo.set_radial; needs segments)."""
        nlay, ncell = nz - 1, (nx - 2) * (ny - 2)
        vel0 = np.ascontiguousarray(vel0, np.float32).reshape(nz, ny, nx)
        vmin, vmax = (np.ascontiguousarray(a, np.float32).reshape(nlay, ny - 2, nx - 2) for a in (vmin, vmax))
        cobs, wdat = (np.ascontiguousarray(a, np.float32).reshape(kmax, ny - 2, nx - 2) for a in (cobs, wdat))
        assert nlay * ncell == vmin.size
        h, ne = C.c_void_p(), C.c_int(0)
        self._check(self.lib.dazim_mc_create(self._h, nx, ny, nz, kmax, int(nchain), int(nbin), C.c_ulonglong(int(seed)), _ptr(vel0),
                                             _ptr(vmin), _ptr(vmax), _ptr(cobs), _ptr(wdat), C.c_float(step), int(nadapt),
                                             C.byref(h), C.byref(ne)))
        mc = MonteCarlo(self, h, nx, ny, nz, kmax, nchain, nbin, ne.value)
        if proposal != 0:
            mc.set_proposal(proposal)
        if ntemp != 1:
            mc.set_tempering(ntemp, tmax, nswap)
        if aniso is not None:
            mc.set_aniso(**aniso)
        if noise is not None:
            mc.set_noise(*noise)
        if prior is not None:
            mc.set_prior(*prior)
        if segments is not None:
            mc.set_segments(segments)
        if noise_groups is not None:
            mc.set_noise_groups(*noise_groups)
        if radial is not None:
            mc.set_radial(radial)
        return mc

    def ray_paths(self):
        """ray geometries of the last rays_build_G call made with option rays.keep_paths = 1: a list of [nrp][2] arrays
        (colatitude, longitude in rad; receiver first, source last) -- the reference's raypath_refmdl_<T>s.dat content"""
        nray, cap = C.c_int64(0), C.c_int(0)
        self._check(self.lib.dazim_ray_paths_dims(self._h, C.byref(nray), C.byref(cap)))
        xz = np.zeros((max(nray.value, 1), max(cap.value, 1), 2), np.float32)
        nrp = np.zeros(max(nray.value, 1), np.int32)
        self._check(self.lib.dazim_ray_paths_copy(self._h, _ptr(xz), _ptr(nrp)))
        if (nrp[:nray.value] < 0).any():
            raise DazimError(DAZIM_E_BAD_ARG, "a ray path outgrew the point buffer")
        return [xz[i, :nrp[i]].copy() for i in range(nray.value)]

    # ---- K6/K7 -----------------------------------------------------------------------------
    def csr_from_coo(self, m, n, irow, icol, rw):
        """COO triplets as the reference holds them (1-based rows iw(2:nar+1), cols, values rw;
        inv/aprod.f90:20-24) -> device CSR + CSC handle"""
        if not _is_torch(rw):
            irow = np.ascontiguousarray(irow, np.int32)
            icol = np.ascontiguousarray(icol, np.int32)
            rw = np.ascontiguousarray(rw, np.float32)
        h = C.c_void_p()
        rc = self.lib.dazim_csr_from_coo(self._h, C.c_int64(m), C.c_int64(n), C.c_int64(int(rw.shape[0])),
                                         _ptr(irow), _ptr(icol), _ptr(rw), C.byref(h))
        self._check(rc)
        return SparseMatrix(self, h, m, n, int(rw.shape[0]))

    def aprod(self, mode, A, x, y):
        """aprod (inv/aprod.f90:7): mode 1: y += A x ; mode 2: x += A^T y (in place)"""
        self._check(self.lib.dazim_aprod(self._h, int(mode), A._h, _ptr(x, np.float32), _ptr(y, np.float32)))

    # ---- N4: what surrounds the solve in the outer iteration -----------------------------------------
    def weight_data(self, G, obst, dsyn, row0=None, dall_glob=None):
        """residual, CalDdatSigma weights (inv/CalSigamNorm.f90:2), weighted right-hand side; scales the data rows of G (nullable).
        numpy in -> (res, datweight, rhs, stats dict)
        row0, dall_glob: dazim_weight_data_sharded -- obst, dsyn are this rank's data rows [row0, row0 + len(obst)) of dall_glob;
        with a communicator attached meandeltaT / stddeltaT and the statistics are those of all data (every rank must call)."""
        obst = np.ascontiguousarray(obst, np.float32); dsyn = np.ascontiguousarray(dsyn, np.float32)
        n = len(obst)
        res, wgt, rhs = (np.zeros(n, np.float32) for _ in range(3))
        st = np.zeros(8, np.float32)
        gh = G._h if G is not None else None
        if row0 is None and dall_glob is None:
            self._check(self.lib.dazim_weight_data(self._h, gh, C.c_int64(n), _ptr(obst), _ptr(dsyn),
                                                   _ptr(res), _ptr(wgt), _ptr(rhs), _ptr(st)))
        else:
            self._check(self.lib.dazim_weight_data_sharded(self._h, gh, C.c_int64(n), C.c_int64(int(row0 or 0)),
                                                           C.c_int64(n if dall_glob is None else int(dall_glob)), _ptr(obst),
                                                           _ptr(dsyn), _ptr(res), _ptr(wgt), _ptr(rhs), _ptr(st)))
        keys = ("mean", "std", "mean_abs", "rms", "meandeltaT", "stddeltaT", "mean_weight", "mean_abs_weighted")
        return res, wgt, rhs, dict(zip(keys, map(float, st)))

    def model_update(self, vs, dv, minvel, maxvel, joint):
        """clamped model update (inv/Main_Jt.f90:582-620); vs[nz][ny][nx] and dv are updated in place (numpy).
        Returns (gc, gs, stats[nblock][nz-1][3])"""
        nz, ny, nx = vs.shape
        maxvp = (nx - 2) * (ny - 2) * (nz - 1)
        nblock = 3 if joint else 1
        assert vs.dtype == np.float32 and dv.dtype == np.float32 and len(dv) == maxvp * nblock
        gc = np.zeros((nz - 1, ny - 2, nx - 2), np.float32) if joint else None
        gs = np.zeros((nz - 1, ny - 2, nx - 2), np.float32) if joint else None
        st = np.zeros((nblock, nz - 1, 3), np.float32)
        self._check(self.lib.dazim_model_update(self._h, nx, ny, nz, int(bool(joint)), _ptr(vs), _ptr(dv), C.c_float(minvel),
                                                C.c_float(maxvel), _ptr(gc), _ptr(gs), _ptr(st)))
        return gc, gs, st

    def lsmr(self, A, b, damp, atol, btol, conlim, itnlim, localSize, x=None, trace_cap=None):
        """LSMR (inv/lsmrModule.f90:36) -> x, info dict (istop, itn, normA, condA, normr, normAr, normx).
        trace_cap: dazim_lsmr_traced with a host array of trace_cap records -> info["trace"] (LSMR_REC, the trace_n records the
        call reports) and info["trace_tail"]: eight more records behind the array's end, filled (like the whole array before
        the call) with the byte LSMR_TRACE_FILL, which the call must leave as they are"""
        if x is None:
            if _is_torch(b):
                import torch
                x = torch.zeros(A.n, dtype=torch.float32, device=b.device)
            else:
                x = np.zeros(A.n, np.float32)
        if not _is_torch(b):
            b = np.ascontiguousarray(b, np.float32)
        istop, itn = C.c_int(0), C.c_int(0)
        sc = [C.c_float(0) for _ in range(5)]
        args = (self._h, A._h, _ptr(b, np.float32), C.c_float(damp), C.c_float(atol), C.c_float(btol),
                C.c_float(conlim), int(itnlim), int(localSize), _ptr(x, np.float32),
                C.byref(istop), C.byref(itn), *[C.byref(s) for s in sc])
        if trace_cap is None:
            self._check(self.lib.dazim_lsmr(*args))
        else:
            cap = int(trace_cap)
            rec = np.empty(max(cap, 0) + 8, LSMR_REC)
            rec.view(np.uint8)[:] = LSMR_TRACE_FILL
            ntr = C.c_int(0)
            self._check(self.lib.dazim_lsmr_traced(*args, C.c_void_p(rec.ctypes.data), cap, C.byref(ntr)))
        info = dict(istop=istop.value, itn=itn.value, normA=sc[0].value, condA=sc[1].value,
                    normr=sc[2].value, normAr=sc[3].value, normx=sc[4].value)
        if trace_cap is not None:
            info["trace"] = rec[:ntr.value]
            info["trace_tail"] = rec[max(cap, 0):]
        return x, info


class MonteCarlo:
    """Metropolis chains of Context.mc_create (dazim_mc): every chain resident on the device"""

    def __init__(self, ctx, handle, nx, ny, nz, kmax, nchain, nbin, n_empty):
        self.ctx, self._h = ctx, handle
        self.nx, self.ny, self.nz, self.kmax, self.nchain, self.nbin, self.n_empty = nx, ny, nz, kmax, nchain, nbin, n_empty
        self.nlay, self.ncell = nz - 1, (nx - 2) * (ny - 2)
        self.ncs = self.ncell - n_empty
        self.ncol = self.ncs * nchain

    def proposals(self):
        """the models the next step evaluates: a torch view [nz][ncol] (fp32, on the context's device) of the handle's array, no
        copy.  The next step overwrites it, and it is invalid once free() has run."""
        import torch
        p, n = C.c_void_p(), C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_mc_proposals(self._h, C.byref(p), C.byref(n)))
        assert n.value == self.ncol
        if n.value == 0:
            return torch.zeros((self.nz, 0), dtype=torch.float32, device=torch.device("cuda", self.ctx.device))

        class _Cai:   # (the CUDA array interface: torch wraps the device pointer without a copy)
            __cuda_array_interface__ = dict(shape=(self.nz, n.value), typestr="<f4", data=(p.value, False), version=2, strides=None)
        return torch.as_tensor(_Cai(), device=torch.device("cuda", self.ctx.device))

    def set_proposal(self, kind):
        """the proposal kind (dazim_mc_set_proposal): 0 isotropic in box units, 1 shaped by the chains' covariance, learnt during
        burn-in and frozen afterwards; refused once a step has been done"""
        self.ctx._check(self.ctx.lib.dazim_mc_set_proposal(self.ctx._h, self._h, int(kind)))

    def cov_state(self):
        """the proposal kind and, for kind 1, copies of the covariance state (dazim_mc_cov_state): dict kind, cov_n[sampled cells],
        cov_s1[sampled cells][nlay], cov_s2, chol[sampled cells][nlay (nlay + 1) / 2] (pair (a, c), c <= a, at a (a + 1) / 2 + c),
        cov_set[sampled cells]; for kind 0 dict kind alone"""
        kind = C.c_int(0)
        self.ctx._check(self.ctx.lib.dazim_mc_cov_state(self.ctx._h, self._h, C.byref(kind), None, None, None, None, None))
        if kind.value != 1:
            return dict(kind=kind.value)
        npair = self.nlay * (self.nlay + 1) // 2
        cov_n = np.zeros(self.ncs, np.int64)
        s1 = np.zeros((self.ncs, self.nlay), np.float64)
        s2 = np.zeros((self.ncs, npair), np.float64)
        chol = np.zeros((self.ncs, npair), np.float64)
        cov_set = np.zeros(self.ncs, np.int32)
        self.ctx._check(self.ctx.lib.dazim_mc_cov_state(self.ctx._h, self._h, None, _ptr(cov_n), _ptr(s1), _ptr(s2), _ptr(chol),
                                                        _ptr(cov_set)))
        return dict(kind=1, cov_n=cov_n, cov_s1=s1, cov_s2=s2, chol=chol, cov_set=cov_set)

    def set_tempering(self, ntemp, tmax, nswap=1):
        """parallel tempering (dazim_mc_set_tempering): chain ch is rung ch % ntemp of replica group ch // ntemp, rung r samples
        the posterior to the power beta_r = tmax ** (-r / (ntemp - 1)), neighbouring rungs swap states every nswap steps and only the
        nchain / ntemp rung-0 chains are recorded; ntemp 1 is the default, no tempering.  Refused once a step has been done"""
        self.ctx._check(self.ctx.lib.dazim_mc_set_tempering(self.ctx._h, self._h, int(ntemp), float(tmax), int(nswap)))

    def temper_state(self):
        """the ladder and, for ntemp > 1, copies of its state (dazim_mc_temper_state): dict ntemp, tmax, nswap, beta[ntemp],
        scale[sampled cells][ntemp], swap_try, swap_acc[sampled cells][ntemp - 1]; for ntemp 1 dict ntemp, tmax, nswap alone"""
        nt, tmax, nswap = C.c_int(0), C.c_float(0), C.c_int(0)
        self.ctx._check(self.ctx.lib.dazim_mc_temper_state(self.ctx._h, self._h, C.byref(nt), C.byref(tmax), C.byref(nswap), None, None,
                                                           None, None))
        out = dict(ntemp=nt.value, tmax=tmax.value, nswap=nswap.value)
        if nt.value == 1:
            return out
        beta = np.zeros(nt.value, np.float64)
        scale = np.zeros((self.ncs, nt.value), np.float32)
        swap_try = np.zeros((self.ncs, nt.value - 1), np.int64)
        swap_acc = np.zeros((self.ncs, nt.value - 1), np.int64)
        self.ctx._check(self.ctx.lib.dazim_mc_temper_state(self.ctx._h, self._h, None, None, None, _ptr(beta), _ptr(scale),
                                                           _ptr(swap_try), _ptr(swap_acc)))
        out.update(beta=beta, scale=scale, swap_try=swap_try, swap_acc=swap_acc)
        return out

    def set_aniso(self, nthin, amap=None, wa=None, smooth=0.0, damp=0.0):
        """Gc/Gs posteriors from the Vs chains (dazim_mc_set_aniso): amap[2][kmax][ny-2][nx-2] = the a1 then a2 maps, wa[kmax][ny-2]
        [nx-2] = 1/sigma_a (0 = no data), smooth and damp those of column_lsq; run() then takes one sample per nthin recorded
        steps.  nthin 0 switches it off again.  Refused once a step has been done"""
        if nthin != 0 and not _is_torch(amap):
            amap = np.ascontiguousarray(amap, np.float32).reshape(2, self.kmax, self.ny - 2, self.nx - 2)
            wa = np.ascontiguousarray(wa, np.float32).reshape(self.kmax, self.ny - 2, self.nx - 2)
        self.ctx._check(self.ctx.lib.dazim_mc_set_aniso(self.ctx._h, self._h, int(nthin), _ptr(amap, np.float32), _ptr(wa, np.float32),
                                                        float(smooth), float(damp)))

    def _ncolc(self):
        nt = C.c_int(0)
        self.ctx._check(self.ctx.lib.dazim_mc_temper_state(self.ctx._h, self._h, C.byref(nt), None, None, None, None, None, None))
        return self.ncs * (self.nchain // nt.value)

    def aniso_step(self, lsen):
        """one Gc/Gs sample (dazim_mc_aniso_step) from lsen[nlay][kmax][ncolc] (fp32; numpy or torch-cuda), the Lsen_Gsc of the
        rung-0 chains' current states in cold-column order (sampled cell, then replica group)"""
        shape = tuple(lsen.shape)
        kmax, ncolc = (shape[1], shape[2]) if len(shape) == 3 and shape[0] == self.nlay else (self.kmax, -1)
        if not _is_torch(lsen):
            lsen = np.ascontiguousarray(lsen, np.float32)
        self.ctx._check(self.ctx.lib.dazim_mc_aniso_step(self.ctx._h, self._h, int(kmax), C.c_int64(int(ncolc)), _ptr(lsen, np.float32)))

    def aniso_state(self):
        """copies of the Gc/Gs sums (dazim_mc_aniso_state): dict nthin, asum[5][nlay][ncolc] (sums of xc, xs, xc^2, xs^2, xc xs),
        avar[nlay][ncolc], acnt[ncolc], skipped; dict nthin alone while it is off"""
        nthin = C.c_int(0)
        self.ctx._check(self.ctx.lib.dazim_mc_aniso_state(self.ctx._h, self._h, C.byref(nthin), None, None, None, None))
        if nthin.value < 1:
            return dict(nthin=nthin.value)
        ncolc = self._ncolc()
        asum = np.zeros((5, self.nlay, ncolc), np.float64)
        avar = np.zeros((self.nlay, ncolc), np.float64)
        acnt = np.zeros(ncolc, np.int64)
        sk = C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_mc_aniso_state(self.ctx._h, self._h, None, _ptr(asum), _ptr(avar), _ptr(acnt), C.byref(sk)))
        return dict(nthin=nthin.value, asum=asum, avar=avar, acnt=acnt, skipped=sk.value)

    def aniso_result(self):
        """Gc/Gs posterior statistics (dazim_mc_aniso_result): dict mean, std, std_between [2][nlay][ny-2][nx-2] (Gc then Gs),
        cov_cs [nlay][ny-2][nx-2], nsamp [ny-2][nx-2]; std_between is the part of std that the Vs uncertainty contributes"""
        shp = (self.nlay, self.ny - 2, self.nx - 2)
        r = dict(mean=np.zeros((2,) + shp, np.float32), std=np.zeros((2,) + shp, np.float32),
                 std_between=np.zeros((2,) + shp, np.float32), cov_cs=np.zeros(shp, np.float32), nsamp=np.zeros(shp[1:], np.int64))
        self.ctx._check(self.ctx.lib.dazim_mc_aniso_result(self.ctx._h, self._h, *(_ptr(r[k]) for k in
                                                                                    ("mean", "std", "std_between", "cov_cs", "nsamp"))))
        return r

    def set_noise(self, a0, b0=1.0):
        """hierarchical data noise (dazim_mc_set_noise): the data std of a cell becomes lambda / w with lambda^2 ~ InverseGamma(a0,
        b0) a priori; lambda is integrated out of the chains' target and its posterior comes back from noise_result().  a0 0 is the
        default, the fixed noise level.  Refused once a step has been done"""
        self.ctx._check(self.ctx.lib.dazim_mc_set_noise(self.ctx._h, self._h, float(a0), float(b0)))

    def noise_state(self):
        """the prior and, while the mode is on, copies of the noise record (dazim_mc_noise_state): dict a0, b0, nsum[2][ncol] (sums
        of sqrt(B) and B over the recorded states), ncnt[ncol]; dict a0 = 0, b0 = 0 alone while it is off"""
        a0, b0 = C.c_float(0), C.c_float(0)
        self.ctx._check(self.ctx.lib.dazim_mc_noise_state(self.ctx._h, self._h, C.byref(a0), C.byref(b0), None, None))
        out = dict(a0=a0.value, b0=b0.value)
        if a0.value == 0:
            return out
        nsum = np.zeros((2, self.ncol), np.float64)
        ncnt = np.zeros(self.ncol, np.int64)
        self.ctx._check(self.ctx.lib.dazim_mc_noise_state(self.ctx._h, self._h, None, None, _ptr(nsum), _ptr(ncnt)))
        out.update(nsum=nsum, ncnt=ncnt)
        return out

    def noise_result(self):
        """the posterior of the noise scale per inner cell (dazim_mc_noise_result): dict lam_mean, lam_std [ny-2][nx-2] (fp32; the
        data std of the cell is lam * sigma) and ndata [ny-2][nx-2] (int32), the cell's periods with data"""
        shp = (self.ny - 2, self.nx - 2)
        r = dict(lam_mean=np.zeros(shp, np.float32), lam_std=np.zeros(shp, np.float32), ndata=np.zeros(shp, np.int32))
        self.ctx._check(self.ctx.lib.dazim_mc_noise_result(self.ctx._h, self._h, *(_ptr(r[k]) for k in ("lam_mean", "lam_std", "ndata"))))
        return r

    def set_noise_groups(self, group_of_period, a0, b0):
        """one noise scale per group of periods (dazim_mc_set_noise_groups): group_of_period[kmax] in 0..G-1, a0, b0[G], G <= 4; the
        data std of a period of group g is lambda_g / w with lambda_g^2 ~ InverseGamma(a0[g], b0[g]), every lambda_g integrated out.
        One group is set_noise(a0[0], b0[0]); every a0 0 is the default, the fixed noise level.  Refused once a step has been done"""
        grp = np.ascontiguousarray(group_of_period, np.int32).ravel()
        a0, b0 = np.ascontiguousarray(a0, np.float32).ravel(), np.ascontiguousarray(b0, np.float32).ravel()
        if len(grp) != self.kmax or len(a0) != len(b0):
            raise DazimError(DAZIM_E_BAD_ARG, f"set_noise_groups: {len(grp)} periods for a handle of {self.kmax}, {len(a0)} a0 and "
                                              f"{len(b0)} b0")
        self.ctx._check(self.ctx.lib.dazim_mc_set_noise_groups(self.ctx._h, self._h, len(a0), _ptr(grp), _ptr(a0), _ptr(b0)))

    def noise_groups_state(self):
        """the groups and, while a noise mode is on, copies of their record (dazim_mc_noise_groups_state): dict ngroup,
        group_of_period[kmax], a0, b0[G], chi2g[G][ncol] (the chi2 of every chain's state per group), nsum[2][G][ncol], ncnt[ncol];
        dict ngroup = 0 alone while it is off"""
        ng = C.c_int(0)
        self.ctx._check(self.ctx.lib.dazim_mc_noise_groups_state(self.ctx._h, self._h, C.byref(ng), None, None, None, None, None, None))
        G = ng.value
        if G == 0:
            return dict(ngroup=0)
        out = dict(ngroup=G, group_of_period=np.zeros(self.kmax, np.int32), a0=np.zeros(G, np.float32), b0=np.zeros(G, np.float32),
                   chi2g=np.zeros((G, self.ncol), np.float64), nsum=np.zeros((2, G, self.ncol), np.float64),
                   ncnt=np.zeros(self.ncol, np.int64))
        self.ctx._check(self.ctx.lib.dazim_mc_noise_groups_state(self.ctx._h, self._h, None, *(_ptr(out[k]) for k in
                                                                 ("group_of_period", "a0", "b0", "chi2g", "nsum", "ncnt"))))
        return out

    def noise_groups_result(self):
        """the posterior of every group's noise scale per inner cell (dazim_mc_noise_groups_result): dict lam_mean, lam_std
        [G][ny-2][nx-2] (fp32) and ndata [G][ny-2][nx-2] (int32), the cell's periods with data in the group"""
        ng = C.c_int(0)
        self.ctx._check(self.ctx.lib.dazim_mc_noise_groups_state(self.ctx._h, self._h, C.byref(ng), None, None, None, None, None, None))
        shp = (max(ng.value, 1), self.ny - 2, self.nx - 2)
        r = dict(lam_mean=np.zeros(shp, np.float32), lam_std=np.zeros(shp, np.float32), ndata=np.zeros(shp, np.int32))
        self.ctx._check(self.ctx.lib.dazim_mc_noise_groups_result(self.ctx._h, self._h, *(_ptr(r[k]) for k in
                                                                                           ("lam_mean", "lam_std", "ndata"))))
        return r

    def set_segments(self, segments):
        """typed data (dazim_mc_set_segments): segments = [(iwave, igr, periods), ...] as Context.dispersion_kernels_typed takes them
        (iwave 1 Love / 2 Rayleigh, igr 0 phase / 1 group; periods an array or its length); the handle's kmax periods are the
        segments' laid end to end, and run() then takes those virtual periods.  [(2, 0, t)] is the default.  Refused once a step has
        been done"""
        iw = np.ascontiguousarray([s[0] for s in segments], np.int32)
        ig = np.ascontiguousarray([s[1] for s in segments], np.int32)
        km = np.ascontiguousarray([s[2] if np.isscalar(s[2]) else len(s[2]) for s in segments], np.int32)
        self.ctx._check(self.ctx.lib.dazim_mc_set_segments(self.ctx._h, self._h, len(segments), _ptr(iw), _ptr(ig), _ptr(km)))

    def set_prior(self, smooth, damp, vref=None):
        """Gaussian smoothness prior (dazim_mc_set_prior): column_lsq's regulariser as a prior of precision smooth^2 L^T L +
        damp^2 I about vref[nz-1][ny-2][nx-2] (None: vel0's knots), truncated by the box; every decision is then taken on the energy
        plus Q = d^T P d.  smooth = damp = 0 is the default, the box alone.  Refused once a step has been done"""
        if vref is not None and not _is_torch(vref):
            vref = np.ascontiguousarray(vref, np.float32).reshape(self.nlay, self.ny - 2, self.nx - 2)
        self.ctx._check(self.ctx.lib.dazim_mc_set_prior(self.ctx._h, self._h, float(smooth), float(damp), _ptr(vref, np.float32)))

    def prior_state(self):
        """the prior and, while it is on, copies of its centre and energies (dazim_mc_prior_state): dict smooth, damp,
        vref[nz-1][ny-2][nx-2], q[ncol] (the Q of the chains' current states); dict smooth = 0, damp = 0 alone while it is off"""
        s, d = C.c_float(0), C.c_float(0)
        self.ctx._check(self.ctx.lib.dazim_mc_prior_state(self.ctx._h, self._h, C.byref(s), C.byref(d), None, None))
        out = dict(smooth=s.value, damp=d.value)
        if s.value == 0 and d.value == 0 and self._radial()[1] == 0:      # (a radial handle's coupling alone keeps the prior on)
            return out
        vref = np.zeros((self.nlay, self.ny - 2, self.nx - 2), np.float32)
        q = np.zeros(self.ncol, np.float64)
        self.ctx._check(self.ctx.lib.dazim_mc_prior_state(self.ctx._h, self._h, None, None, _ptr(vref), _ptr(q)))
        out.update(vref=vref, q=q)
        return out

    def set_radial(self, couple):
        """radial anisotropy (dazim_mc_set_radial): the handle's knots are the stacked vector [Vsv_0..Vsv_{n-1}, Vsh_0..Vsh_{n-1},
        deepest] (create it with nz = 2n + 1), run() computes the Rayleigh segments' curves from the Vsv model and the Love segments'
        from the Vsh model (depz then has n + 1 entries), the prior gains couple^2 |Vsh - Vsv|^2, and every recorded state adds
        xi = (Vsh / Vsv)^2, the Voigt average and Vsv Vsh to the radial record.  Needs set_segments with Rayleigh before Love;
        refused once a step has been done"""
        self.ctx._check(self.ctx.lib.dazim_mc_set_radial(self.ctx._h, self._h, float(couple)))

    def _radial(self):
        n, c = C.c_int(0), C.c_float(0)
        self.ctx._check(self.ctx.lib.dazim_mc_radial_state(self.ctx._h, self._h, C.byref(n), C.byref(c), None, None, None))
        return n.value, c.value

    def radial_models(self):
        """the two models run()'s dispersion calls read (dazim_mc_radial_models): torch views (vsv, vsh), each [n+1][ncol] (fp32, on
        the context's device), no copy; valid after set_radial and after every step, invalid once free() has run"""
        import torch
        pv, ph, nc = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_mc_radial_models(self._h, C.byref(pv), C.byref(ph), C.byref(nc)))
        n = self.nlay // 2
        dev = torch.device("cuda", self.ctx.device)
        if nc.value == 0:
            return tuple(torch.zeros((n + 1, 0), dtype=torch.float32, device=dev) for _ in range(2))

        def view(p):
            class _Cai:
                __cuda_array_interface__ = dict(shape=(n + 1, nc.value), typestr="<f4", data=(p.value, False), version=2, strides=None)
            return torch.as_tensor(_Cai(), device=dev)
        return view(pv), view(ph)

    def radial_state(self):
        """the radial mode and, while it is on, copies of its record (dazim_mc_radial_state): dict n, couple, rsum[5][n][ncol] (sums
        of xi, xi^2, Vsv Vsh, V, V^2), ngt1[n][ncol] (states with xi > 1), xhist[sampled cells][n][nbin]; dict n = 0, couple = 0
        alone on a handle that is not radial"""
        n, c = self._radial()
        out = dict(n=n, couple=c)
        if n == 0:
            return out
        rsum = np.zeros((5, n, self.ncol), np.float64)
        ngt1 = np.zeros((n, self.ncol), np.int64)
        xhist = np.zeros((self.ncs, n, self.nbin), np.uint32)
        self.ctx._check(self.ctx.lib.dazim_mc_radial_state(self.ctx._h, self._h, None, None, _ptr(rsum), _ptr(ngt1), _ptr(xhist)))
        out.update(rsum=rsum, ngt1=ngt1, xhist=xhist)
        return out

    def radial_result(self):
        """posterior statistics of the derived quantities (dazim_mc_radial_result): dict xi_mean, xi_std, xi_rhat, p_gt1 (the
        posterior probability of xi > 1), corr_vh (the Vsv-Vsh correlation), voigt_mean, voigt_std [n][ny-2][nx-2] and xi_q
        [3][n][ny-2][nx-2] (2.5 / 50 / 97.5 %)"""
        shp = (self.nlay // 2, self.ny - 2, self.nx - 2)
        keys = ("xi_mean", "xi_std", "xi_q", "xi_rhat", "p_gt1", "corr_vh", "voigt_mean", "voigt_std")
        r = {k: np.zeros(((3,) if k == "xi_q" else ()) + shp, np.float32) for k in keys}
        self.ctx._check(self.ctx.lib.dazim_mc_radial_result(self.ctx._h, self._h, *(_ptr(r[k]) for k in keys)))
        return r

    def step(self, pv, record):
        """one step on pv[kmax][ncol] (fp64; numpy or torch-cuda), the curves of proposals(); record 0 = burn-in"""
        shape = tuple(pv.shape)
        kmax, ncol = (shape[0], shape[1]) if len(shape) == 2 else (self.kmax, -1)
        if not _is_torch(pv):
            pv = np.ascontiguousarray(pv, np.float64)
        self.ctx._check(self.ctx.lib.dazim_mc_step(self.ctx._h, self._h, int(kmax), C.c_int64(int(ncol)), _ptr(pv, np.float64),
                                                   int(record)))

    def run(self, depz, sublayers, periods, nburn, nsample):
        """nburn burn-in and nsample recorded steps with the dispersion forward model (dazim_mc_run); returns the proposals without
        a root.  After set_segments, periods are the virtual periods, segment after segment; after set_radial depz has the n + 1
        knot depths of one profile"""
        depz = np.ascontiguousarray(depz, np.float32)
        periods = np.ascontiguousarray(periods, np.float64)
        nrad = self._radial()[0]
        assert len(depz) == (nrad + 1 if nrad else self.nz) and len(periods) == self.kmax
        nr = C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_mc_run(self.ctx._h, self._h, _ptr(depz), C.c_float(sublayers), _ptr(periods), int(nburn),
                                                  int(nsample), C.byref(nr)))
        return nr.value

    def state(self):
        """copies of the chain state: dict cur[nz][ncol], chi2[ncol], scale[sampled cells], step, sums[2][nlay][ncol],
        hist[sampled cells][nlay][nbin], accepted[ncol], best[nlay][sampled cells], best_chi2[sampled cells]"""
        cur = np.zeros((self.nz, self.ncol), np.float32)
        chi2 = np.zeros(self.ncol, np.float64)
        scale = np.zeros(self.ncs, np.float32)
        sums = np.zeros((2, self.nlay, self.ncol), np.float64)
        hist = np.zeros((self.ncs, self.nlay, self.nbin), np.uint32)
        acc = np.zeros(self.ncol, np.int64)
        best = np.zeros((self.nlay, self.ncs), np.float32)
        best_chi2 = np.zeros(self.ncs, np.float64)
        st = C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_mc_state(self.ctx._h, self._h, _ptr(cur), _ptr(chi2), _ptr(scale), C.byref(st), _ptr(sums),
                                                    _ptr(hist), _ptr(acc), _ptr(best), _ptr(best_chi2)))
        return dict(cur=cur, chi2=chi2, scale=scale, step=st.value, sums=sums, hist=hist, accepted=acc, best=best, best_chi2=best_chi2)

    def result(self):
        """posterior statistics: dict mean, std, best, rhat [nlay][ny-2][nx-2], q [3][nlay][ny-2][nx-2], accept, chi2_best
        [ny-2][nx-2]"""
        shp = (self.nlay, self.ny - 2, self.nx - 2)
        r = dict(mean=np.zeros(shp, np.float32), std=np.zeros(shp, np.float32), q=np.zeros((3,) + shp, np.float32),
                 best=np.zeros(shp, np.float32), rhat=np.zeros(shp, np.float32), accept=np.zeros(shp[1:], np.float32),
                 chi2_best=np.zeros(shp[1:], np.float32))
        self.ctx._check(self.ctx.lib.dazim_mc_result(self.ctx._h, self._h, *(_ptr(r[k]) for k in
                                                                              ("mean", "std", "q", "best", "rhat", "accept", "chi2_best"))))
        return r

    def free(self):
        if self._h:
            self.ctx.lib.dazim_mc_free(self.ctx._h if self.ctx._h else None, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SparseMatrix:
    """device-resident G (dazim_csr)"""

    def __init__(self, ctx, handle, m, n, nnz):
        self.ctx, self._h, self.m, self.n, self.nnz = ctx, handle, m, n, nnz

    def scale_rows(self, w):
        self.ctx._check(self.ctx.lib.dazim_csr_scale_rows(self.ctx._h, self._h, _ptr(w, np.float32)))

    def append_coo(self, extra_m, irow, icol, rw):
        """append rows m+1..m+extra_m (absolute 1-based ids) -- Tikhonov rows, inv/TikhRegul.f90:2"""
        irow = np.ascontiguousarray(irow, np.int32); icol = np.ascontiguousarray(icol, np.int32)
        rw = np.ascontiguousarray(rw, np.float32)
        self.ctx._check(self.ctx.lib.dazim_csr_append_coo(self.ctx._h, self._h, C.c_int64(extra_m), C.c_int64(len(rw)),
                                                          _ptr(irow), _ptr(icol), _ptr(rw)))
        self.m += extra_m
        self.nnz += len(rw)

    def append_tikhonov(self, nx, ny, nz, weights):
        """Tikhonov rows generated on the device (inv/TikhRegul.f90:2): one block of (nx-2)(ny-2)(nz-1) rows per weight"""
        w = np.ascontiguousarray(weights, np.float32)
        m0, z0 = C.c_int64(0), C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_csr_append_tikhonov(self.ctx._h, self._h, nx, ny, nz, len(w), _ptr(w)))
        self.ctx._check(self.ctx.lib.dazim_csr_dims(self._h, C.byref(m0), None, C.byref(z0)))
        self.m, self.nnz = m0.value, z0.value

    def append_tikhonov_rows(self, nx, ny, nz, weights, row_lo, row_hi):
        """rows [row_lo, row_hi) of the len(weights) * (nx-2)(ny-2)(nz-1) rows of append_tikhonov (dazim_csr_append_tikhonov_rows):
        the share of one rank of a row-sharded system"""
        w = np.ascontiguousarray(weights, np.float32)
        m0, z0 = C.c_int64(0), C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_csr_append_tikhonov_rows(self.ctx._h, self._h, nx, ny, nz, len(w), _ptr(w),
                                                                    C.c_int64(row_lo), C.c_int64(row_hi)))
        self.ctx._check(self.ctx.lib.dazim_csr_dims(self._h, C.byref(m0), None, C.byref(z0)))
        self.m, self.nnz = m0.value, z0.value

    def append_laplacian2d(self, nx, ny, weights):
        """2-D regularisation rows of the per-period maps generated on the device (dazim_csr_append_laplacian2d): one block of
        (nx-2)(ny-2) rows per weight, map b regularising columns b*ncell .."""
        w = np.ascontiguousarray(weights, np.float32)
        m0, z0 = C.c_int64(0), C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_csr_append_laplacian2d(self.ctx._h, self._h, nx, ny, len(w), _ptr(w)))
        self.ctx._check(self.ctx.lib.dazim_csr_dims(self._h, C.byref(m0), None, C.byref(z0)))
        self.m, self.nnz = m0.value, z0.value

    def take_twin(self):
        """the dense twin (the reference's GVs | GGc | GGs) of a matrix built with option rays.dense_twin = 1, or None"""
        h = C.c_void_p()
        self.ctx._check(self.ctx.lib.dazim_csr_take_twin(self.ctx._h, self._h, C.byref(h)))
        if not h.value:
            return None
        m0, z0 = C.c_int64(0), C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_csr_dims(h, C.byref(m0), None, C.byref(z0)))
        return SparseMatrix(self.ctx, h, m0.value, self.n, z0.value)

    def threshold(self, tol, reserve_rows=0, reserve_nnz=0):
        """a new matrix holding the entries with |value| > tol (dazim_csr_threshold): the solver's triplets (inv/CalSurfG.f90:1358)
        from a matrix built with option rays.keep_small (the entries of the reference's dense GVs/GGc/GGs, :1369-1378)"""
        h = C.c_void_p()
        self.ctx._check(self.ctx.lib.dazim_csr_threshold(self.ctx._h, self._h, C.c_float(tol), C.c_int64(reserve_rows),
                                                         C.c_int64(reserve_nnz), C.byref(h)))
        m0, z0 = C.c_int64(0), C.c_int64(0)
        self.ctx._check(self.ctx.lib.dazim_csr_dims(h, C.byref(m0), None, C.byref(z0)))
        return SparseMatrix(self.ctx, h, m0.value, self.n, z0.value)

    def col_abs_sums(self):
        """DWS, norm(col) = sum |rw| over the column's entries (inv/Main_Jt.f90:477-481, dazim_csr_col_abs_sums) -> fp32 [n]"""
        out = np.zeros(self.n, np.float32)
        self.ctx._check(self.ctx.lib.dazim_csr_col_abs_sums(self.ctx._h, self._h, _ptr(out)))
        return out

    def to_coo(self):
        irow = np.zeros(self.nnz, np.int32); icol = np.zeros(self.nnz, np.int32); rw = np.zeros(self.nnz, np.float32)
        self.ctx._check(self.ctx.lib.dazim_csr_to_coo(self.ctx._h, self._h, _ptr(irow), _ptr(icol), _ptr(rw)))
        return irow, icol, rw

    def free(self):
        """release the device arrays (also done when the object is collected; safe after the context was closed)"""
        if self._h:
            self.ctx.lib.dazim_csr_free(self.ctx._h if self.ctx._h else None, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
