"""-m gpu: the second step of the two-step method on the device (dazim_vs_kernels, dazim_column_lsq).

The per-cell solver is compared with numpy.linalg.lstsq of the stacked fp64 system [diag(w) K; smooth L; damp I] x = [w r; 0; 0],
dazim_vs_kernels with a NumPy transcription of k_row_kernels and, bit for bit, with the entries of the 3-D rows, and the pieces
together with a noise-free synthetic recovery of Vs and of Gc/Gs."""
import ctypes as C

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import synth
from tests.bars import within
from tests.test_phase_maps_gpu import DV, GOXD, GOZD, survey

pytestmark = pytest.mark.gpu


def depth_rule(n):
    """L of the issue: TikhRegul's rule restricted to depth -- the first and last knot the single entry 2, an inner knot 2, -1, -1"""
    L = np.zeros((n, n))
    for i in range(n):
        L[i, i] = 2.0
        if 0 < i < n - 1:
            L[i, i - 1] = L[i, i + 1] = -1.0
    return L


def lsq_numpy(nx, ny, nlay, kern, rhs, wdat, smooth, damp):
    """every cell's problem as one stacked fp64 least-squares system; x [nrhs][nlay][ncell], the cells without data left at 0, and
    the RMS over the cells with w != 0 of r and of r - K x per (right-hand side, period)"""
    nrhs, kmax = rhs.shape[0], kern.shape[1]
    nvx, ncell = nx - 2, (nx - 2) * (ny - 2)
    s, d = float(np.float32(smooth)), float(np.float32(damp))
    L = depth_rule(nlay)
    x = np.zeros((nrhs, nlay, ncell))
    ss = np.zeros((nrhs, kmax, 2))
    cnt = np.zeros(kmax)
    r = rhs.reshape(nrhs, kmax, ncell).astype(np.float64)
    w = wdat.reshape(kmax, ncell).astype(np.float64)
    for c in range(ncell):
        col = (c // nvx + 1) * nx + c % nvx + 1
        if not (w[:, c] != 0).any():
            continue
        K = kern[:nlay, :, col].T.astype(np.float64)
        A = np.vstack([w[:, c, None] * K, s * L, d * np.eye(nlay)])
        on = w[:, c] != 0
        cnt += on
        for q in range(nrhs):
            b = np.concatenate([w[:, c] * r[q, :, c], np.zeros(2 * nlay)])
            x[q, :, c] = np.linalg.lstsq(A, b, rcond=None)[0]
            res = r[q, :, c] - K @ x[q, :, c]
            ss[q, on, 0] += r[q, on, c] ** 2
            ss[q, on, 1] += res[on] ** 2
    return x, np.sqrt(ss / np.maximum(cnt, 1)[None, :, None])


def random_problem(nx, ny, nlay, kmax, nrhs, fp32, seed):
    rng = np.random.default_rng(seed)
    ncell = (nx - 2) * (ny - 2)
    kern = rng.standard_normal((nlay + 1, kmax, nx * ny)).astype(np.float32 if fp32 else np.float64)   # (one layer too many: unread)
    rhs = rng.standard_normal((nrhs, kmax, ny - 2, nx - 2)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, (kmax, ncell)).astype(np.float32)
    w[rng.random((kmax, ncell)) < 0.25] = 0.0
    w[:, 3] = 0.0                                  # a cell without data
    w[:, 5] = 0.0
    w[kmax - 1, 5] = 1.0                           # ... and one with a single period
    return kern, rhs, w.reshape(kmax, ny - 2, nx - 2)


@pytest.mark.parametrize("reg", [(0.7, 0.3), (0.0, 0.5), (0.8, 0.0)], ids=["smooth+damp", "damp", "smooth"])
@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nrhs", [1, 2])
@pytest.mark.parametrize("kmax", [1, 4, 16, 60])
@pytest.mark.parametrize("nlay", [1, 2, 11, 19, 63])
def test_column_lsq_equals_numpy_lstsq(ctx, nlay, kmax, nrhs, fp32, reg):
    """x within 1e-6 * max(1, max |x_np|) of lstsq in every cell, 0 exactly in the cell without data (counted in n_empty), the RMS
    statistics within 1e-5 relative; device (torch) arrays give the bits of host arrays"""
    import torch
    nx, ny = 7, 6
    smooth, damp = reg
    kern, rhs, w = random_problem(nx, ny, nlay, kmax, nrhs, fp32, seed=nlay * 1000 + kmax * 10 + nrhs)
    x, ne, st = ctx.column_lsq(nx, ny, nlay, kern, rhs, w, smooth, damp)
    xn, stn = lsq_numpy(nx, ny, nlay, kern, rhs, w, smooth, damp)
    empty = ~(w.reshape(kmax, -1) != 0).any(axis=0)
    assert empty[3] and ne == int(empty.sum()) and x.shape == (nrhs, nlay, ny - 2, nx - 2)
    xc = x.reshape(nrhs, nlay, -1)
    assert (xc[:, :, empty] == 0).all()
    err = np.abs(xc - xn).max(axis=(0, 1)) / np.maximum(1.0, np.abs(xn).max(axis=(0, 1)))
    assert err.max() <= 1e-6, err.max()
    assert np.allclose(st, stn, rtol=1e-5, atol=0), np.abs(st - stn).max()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, ned, std = ctx.column_lsq(nx, ny, nlay, T(kern), T(rhs), T(w), smooth, damp)
    assert ned == ne and np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))
    assert np.array_equal(std.view(np.uint32), st.view(np.uint32))


def test_column_lsq_without_weights_is_all_ones(ctx):
    nx, ny, nlay, kmax = 9, 8, 5, 7
    kern, rhs, _ = random_problem(nx, ny, nlay, kmax, 2, 0, seed=4)
    x, ne, st = ctx.column_lsq(nx, ny, nlay, kern, rhs, None, 0.5, 0.1)
    x1, ne1, st1 = ctx.column_lsq(nx, ny, nlay, kern, rhs, np.ones((kmax, ny - 2, nx - 2), np.float32), 0.5, 0.1)
    assert ne == ne1 == 0 and np.array_equal(x, x1) and np.array_equal(st, st1)


@pytest.mark.parametrize("bad", ["nlay0", "nlay64", "kmax0", "kmax61", "nrhs0", "nrhs3", "smooth<0", "damp<0", "both0"])
def test_column_lsq_refusals(ctx, bad):
    """each refusal of the issue returns DAZIM_E_BAD_ARG (the raw entry, with buffers large enough for any of the calls)"""
    nx, ny = 5, 5
    a = dict(nlay=3, kmax=4, nrhs=1, smooth=1.0, damp=0.5)
    a.update({"nlay0": dict(nlay=0), "nlay64": dict(nlay=64), "kmax0": dict(kmax=0), "kmax61": dict(kmax=61), "nrhs0": dict(nrhs=0),
              "nrhs3": dict(nrhs=3), "smooth<0": dict(smooth=-0.1), "damp<0": dict(damp=-1e-3),
              "both0": dict(smooth=0.0, damp=0.0)}[bad])
    kern = np.zeros(64 * 61 * nx * ny)
    rhs = np.zeros(3 * 61 * 9, np.float32)
    x = np.zeros(3 * 64 * 9, np.float32)
    ne = C.c_int(0)
    rc = ctx.lib.dazim_column_lsq(ctx._h, nx, ny, a["nlay"], a["kmax"], 0, C.c_void_p(kern.ctypes.data), a["nrhs"],
                                  C.c_void_p(rhs.ctypes.data), None, C.c_float(a["smooth"]), C.c_float(a["damp"]),
                                  C.c_void_p(x.ctypes.data), C.byref(ne), None)
    assert rc == dz.DAZIM_E_BAD_ARG
    assert ctx.lib.dazim_column_lsq(ctx._h, nx, ny, 3, 4, 0, C.c_void_p(kern.ctypes.data), 1, C.c_void_p(rhs.ctypes.data), None,
                                    C.c_float(1.0), C.c_float(0.5), C.c_void_p(x.ctypes.data), C.byref(ne), None) == 0


def row_kernels_numpy(vel, sen):
    """k_row_kernels restated: svp*coe_a + srho*coe_rho + svs with the Brocher derivatives of the cell's velocity in fp32"""
    nz, ny, nx = vel.shape
    f = np.float32
    v = vel.reshape(nz, 1, nx * ny).astype(f)
    coe_a = f(2.0947) - f(0.8206) * f(2) * v + f(0.2683) * f(3) * (v * v) - f(0.0251) * f(4) * (v * v * v)
    vp = f(0.9409) + f(2.0947) * v - f(0.8206) * (v * v) + f(0.2683) * (v * v * v) - f(0.0251) * (v * v * v * v)
    coe_rho = coe_a * (f(1.6612) - f(0.4721) * f(2) * vp + f(0.0671) * f(3) * (vp * vp) - f(0.0043) * f(4) * (vp * vp * vp)
                       + f(0.000106) * f(5) * (vp * vp * vp * vp))
    return sen[1] * coe_a.astype(np.float64) + sen[2] * coe_rho.astype(np.float64) + sen[0]


def layered_model(nx, ny, depz, seed, amp=0.15):
    """Vs increasing with depth plus smooth lateral perturbations of +-amp km/s, the deepest knot laterally uniform"""
    rng = np.random.default_rng(seed)
    nz = len(depz)
    mean = 2.9 + 1.6 * np.asarray(depz, np.float64) / max(depz[-1], 1.0)
    vel = np.empty((nz, ny, nx), np.float32)
    for k in range(nz):
        n = synth.smooth_noise(rng, (ny, nx))
        vel[k] = mean[k] + (amp * n / np.abs(n).max() if k < nz - 1 else 0.0)
    return vel


def test_vs_kernels_is_the_table_the_3d_rows_multiply(ctx):
    """dazim_vs_kernels on dazim_dispersion_kernels' tables: within 1e-6 relative of the NumPy transcription, and every entry of
    the iso rows (rays.keep_small = 1) of layer k is (float)(skern[k] * (double)fdm) bit for bit, fdm the map row entry of the
    same ray and cell"""
    nx, ny, kmax = 17, 15, 3
    depz = np.array([0.0, 5.0, 15.0, 30.0, 50.0], np.float32)
    nz, ncell, nvx = len(depz), (nx - 2) * (ny - 2), nx - 2
    tRc = np.array([8.0, 15.0, 25.0])
    vel = layered_model(nx, ny, depz, seed=5)
    pv, sen, nf = ctx.depthkernel(vel, depz, tRc, 2.0)
    assert nf == 0
    skern = ctx.vs_kernels(vel, sen)
    ref = row_kernels_numpy(vel, sen)
    within("vs_kernels vs NumPy k_row_kernels, max relative", np.abs(skern - ref).max() / np.abs(ref).max(), 1e-6)
    scx, scz, per, ray_f, rx, rz = survey(nx, ny, kmax, 8, 7, seed=3)
    ctx.set_option("rays.keep_small", 1)
    try:
        G3, _, _ = ctx.rays_build_G(nx, ny, GOXD, GOZD, DV, DV, vel, ctx.fmm_batch(nx, ny, GOXD, GOZD, DV, DV, pv, scx, scz, per),
                                    scx, scz, per, ray_f, rx, rz, sen)
        Gm, _, _ = ctx.rays_build_G_maps(nx, ny, GOXD, GOZD, DV, DV, ctx.fmm_batch(nx, ny, GOXD, GOZD, DV, DV, pv, scx, scz, per),
                                         scx, scz, per, ray_f, rx, rz)
    finally:
        ctx.set_option("rays.keep_small", 0)
    ir3, ic3, rw3 = G3.to_coo()
    irm, icm, rwm = Gm.to_coo()
    G3.free(); Gm.free()
    key_m = (irm.astype(np.int64) - 1) * ncell + (icm - 1) % ncell
    order = np.argsort(key_m)
    key_m, fdm = key_m[order], rwm[order]
    assert len(np.unique(key_m)) == len(key_m)
    layer, cell = (ic3 - 1) // ncell, (ic3 - 1) % ncell
    key3 = (ir3.astype(np.int64) - 1) * ncell + cell
    pos = np.searchsorted(key_m, key3)
    assert (pos < len(key_m)).all() and np.array_equal(key_m[pos], key3)      # every iso entry has its map entry
    kslot = per[ray_f[ir3 - 1]] - 1
    col = (cell // nvx + 1) * nx + cell % nvx + 1
    want = (skern[layer, kslot, col] * fdm[pos].astype(np.float64)).astype(np.float32)
    assert len(rw3) > 1000 and set(np.unique(layer)) == set(range(nz - 1))
    assert np.array_equal(rw3.view(np.uint32), want.view(np.uint32))


def rms_misfit(pv, c_true, nx, ny):
    d = (pv - c_true).reshape(-1, ny, nx)[:, 1:-1, 1:-1]
    return float(np.sqrt(np.mean(d ** 2)))


def test_synthetic_recovery_vs_then_gc_gs(ctx):
    """12 x 12 columns, 8 knots, 12 periods, noise-free: from the layer means, 4 linearised iterations dispersion -> vs_kernels ->
    column_lsq -> model_update lower the RMS c misfit every time and end below 10 % of its start; then Gc, Gs from a1, a2 = sum_k
    Lsen Gc (Gs) of a true model fit a1, a2 to 1e-4 relative RMS with a small smoothing (1e-5; measured on an MI355X with 1e-3:
    7.3e-4, the smoothing's bias on a1, a2 of a few 1e-3 km/s).  Measured: c misfit 0.0308 -> 0.0005 km/s (1.6 %), RMS Vs error
    0.057 -> 0.036 km/s."""
    nx = ny = 14
    depz = np.array([0.0, 4.0, 10.0, 18.0, 28.0, 40.0, 55.0, 75.0], np.float32)
    tRc = np.array([5.0, 7.0, 9.0, 12.0, 15.0, 19.0, 24.0, 30.0, 36.0, 43.0, 50.0, 60.0])
    nz, kmax, nlay = len(depz), len(tRc), len(depz) - 1
    true = layered_model(nx, ny, depz, seed=9)
    c_true, _, nf = ctx.depthkernel(true, depz, tRc, 2.0, kernels=False)
    assert nf == 0
    vs = np.broadcast_to(true.mean(axis=(1, 2), keepdims=True), true.shape).astype(np.float32).copy()
    misfit = []
    for it in range(4):
        pv, sen, nf = ctx.depthkernel(vs, depz, tRc, 2.0)
        assert nf == 0
        misfit.append(rms_misfit(pv, c_true, nx, ny))
        skern = ctx.vs_kernels(vs, sen)
        r = (c_true - pv).reshape(kmax, ny, nx)[:, 1:-1, 1:-1].astype(np.float32)
        x, ne, st = ctx.column_lsq(nx, ny, nlay, skern, r[None], None, 0.05, 0.01)
        assert ne == 0
        assert abs(np.sqrt(np.mean(st[0, :, 0] ** 2)) - misfit[-1]) <= 1e-4 * misfit[-1]
        ctx.model_update(vs, x.reshape(-1).copy(), 2.0, 5.0, False)
    pv, _, _ = ctx.depthkernel(vs, depz, tRc, 2.0, kernels=False)
    misfit.append(rms_misfit(pv, c_true, nx, ny))
    print("\n[measured] RMS c misfit per iteration (km/s): " + " ".join("%.5f" % m for m in misfit))
    assert all(b < a for a, b in zip(misfit, misfit[1:])), misfit
    within("final / starting RMS c misfit", misfit[-1] / misfit[0], 0.1)
    err_start = np.sqrt(np.mean((true.mean(axis=(1, 2))[:-1, None, None] - true[:-1]) ** 2))
    err_end = np.sqrt(np.mean((vs[:-1, 1:-1, 1:-1] - true[:-1, 1:-1, 1:-1]) ** 2))
    print("[measured] RMS Vs error start %.4f -> recovered %.4f km/s" % (err_start, err_end))
    # Gc / Gs on the final Vs
    lsen = ctx.ti_kernels(vs, depz, tRc, 2.0, pv)
    rng = np.random.default_rng(12)
    g = np.stack([0.03 * synth.smooth_noise(rng, (nlay, ny - 2, nx - 2)) for _ in range(2)])   # [2][nlay][ny-2][nx-2]
    L = lsen.reshape(nlay, kmax, ny, nx)[:, :, 1:-1, 1:-1].astype(np.float64)
    a = np.einsum("ktji,qkji->qtji", L, g).astype(np.float32)                                   # a1, a2 [2][kmax][ny-2][nx-2]
    x, ne, st = ctx.column_lsq(nx, ny, nlay, lsen, a, None, 1e-5, 0.0)
    pred = np.einsum("ktji,qkji->qtji", L, x.astype(np.float64))
    rel = np.sqrt(np.mean((pred - a) ** 2)) / np.sqrt(np.mean(a.astype(np.float64) ** 2))
    within("a1, a2 refit from the recovered Gc, Gs, relative RMS", rel, 1e-4)
