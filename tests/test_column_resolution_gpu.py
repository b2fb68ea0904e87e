"""-m gpu: dazim_column_resolution: posterior std, resolution matrix and what is derived from it, per inner cell
and knot, from the Cholesky factor of dazim_column_lsq's normal matrix.

Against numpy.linalg (tests/column_res_ref.py) over the shapes of the column solve's own test, against the solve itself (noise-free
data: x = Rm z), the bounds any definite regulariser implies, the Monte-Carlo pass's conditional variance (the same inverse factor),
the refused calls and the special cells.  nx = 7, ny = 6: 20 cells, random_problem's cell without data and its single-period cell.
The largest LDS request (nlay 63, kmax 60, rows on: 94 224 bytes) is a case of the first test.
Measured on an MI355X against numpy.linalg, largest over the 90 cases: std_post 5.5e-8, std_noise 4.1e-8, rdiag 5.2e-8, rsum 6.3e-8,
width 5.5e-8, rows 5.5e-8, trace 5.4e-8 (bar 1e-6); float32(sqrt(avar)) against std_post 0 ulp in 490 values."""
import ctypes as C
import functools

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import column_res_ref as ref
from tests.bars import within
from tests.test_column_lsq_gpu import random_problem
from tests.test_column_mc_aniso_gpu import curves, grid_problem, trend_kernels, ulps

pytestmark = pytest.mark.gpu

NX, NY = 7, 6
NCELL = (NX - 2) * (NY - 2)
REGS = [(0.7, 0.3), (0.0, 0.5), (0.8, 0.0)]
REG_IDS = ["smooth+damp", "damp", "smooth"]
PER_KNOT = ("std_post", "std_noise", "rdiag", "rsum")


@functools.lru_cache(maxsize=None)
def problem(nlay, kmax, fp32):
    kern, _, w = random_problem(NX, NY, nlay, kmax, 1, fp32, seed=nlay * 1000 + kmax * 10 + 1)
    for a in (kern, w):
        a.setflags(write=False)
    return kern, w, ref.knot_depths(nlay)


@functools.lru_cache(maxsize=None)
def reference(nlay, kmax, fp32, reg):
    kern, w, depz = problem(nlay, kmax, fp32)
    return ref.per_cell(ref.linalg, NX, NY, nlay, kern, w, *reg, depz)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kmax", [1, 4, 60])
@pytest.mark.parametrize("nlay", [1, 2, 3, 11, 63])
def test_equals_numpy_linalg(ctx, nlay, kmax, fp32, reg):
    """every output within 1e-6 * max(1, max |reference|) of numpy.linalg per cell; the cell without data 0 in every output and
    counted; torch device arrays give the bits of host arrays; leaving out rows or depz changes no bit of the rest"""
    import torch
    kern, w, depz = problem(nlay, kmax, fp32)
    want = reference(nlay, kmax, fp32, reg)
    got = ctx.column_resolution(NX, NY, nlay, kern, w, *reg, depz=depz, rows=True)
    empty = ~(w.reshape(kmax, -1) != 0).any(axis=0)
    assert empty[3] and got["n_empty"] == int(empty.sum()) == want["n_empty"] and got["n_failed"] == 0
    assert got["rows"].shape == (nlay, nlay, NY - 2, NX - 2) and got["trace"].shape == (NY - 2, NX - 2)
    for k in ref.OUTPUTS:
        assert got[k].dtype == np.float32 and not bits(got[k]).reshape(-1, NCELL)[:, empty].any(), k
    for k, v in ref.worst(got, want).items():
        within(f"column_resolution vs numpy.linalg, {k}, nlay {nlay} kmax {kmax}", v, 1e-6)
    T = lambda a: torch.from_numpy(np.array(a)).cuda()
    dev = ctx.column_resolution(NX, NY, nlay, T(kern), T(w), *reg, depz=T(depz), rows=True)
    assert (dev["n_empty"], dev["n_failed"]) == (got["n_empty"], 0)
    for k in ref.OUTPUTS:
        assert np.array_equal(bits(dev[k].cpu().numpy()), bits(got[k])), k
    lean = ctx.column_resolution(NX, NY, nlay, kern, w, *reg)
    assert lean["rows"] is None and lean["width"] is None
    for k in PER_KNOT + ("trace",):
        assert np.array_equal(bits(lean[k]), bits(got[k])), k


def test_without_weights_is_all_ones(ctx):
    nlay, kmax = 5, 7
    kern, _, depz = problem(nlay, kmax, 0)
    a = ctx.column_resolution(NX, NY, nlay, kern, None, 0.5, 0.1, depz=depz, rows=True)
    b = ctx.column_resolution(NX, NY, nlay, kern, np.ones((kmax, NY - 2, NX - 2), np.float32), 0.5, 0.1, depz=depz, rows=True)
    assert a["n_empty"] == b["n_empty"] == 0
    for k in ref.OUTPUTS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nlay", [1, 2, 3, 11, 63])
def test_it_is_the_solves_resolution(ctx, nlay, fp32):
    """integer K (|K| <= 8), integer z (|z| <= 4), weights that are powers of two: r = K z is exact in fp32, so dazim_column_lsq's x
    for it is Rm z: x against rows @ z (rows widened to fp64) within 1e-6 * max(1, max |rows @ z|) per cell"""
    kmax = 12
    rng = np.random.default_rng(77 + nlay)
    kern = rng.integers(-8, 9, (nlay, kmax, NX * NY)).astype(np.float32 if fp32 else np.float64)
    z = rng.integers(-4, 5, (nlay, NCELL)).astype(np.float64)
    w = (2.0 ** rng.integers(-1, 2, (kmax, NCELL))).astype(np.float32)
    w[rng.random((kmax, NCELL)) < 0.25] = 0.0
    w[:, 3] = 0.0
    Kc = kern.reshape(nlay, kmax, NY, NX)[:, :, 1:-1, 1:-1].reshape(nlay, kmax, NCELL).astype(np.float64)
    r = np.einsum("lpc,lc->pc", Kc, z)
    r32 = r.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), r)
    w = w.reshape(kmax, NY - 2, NX - 2)
    x, ne, _ = ctx.column_lsq(NX, NY, nlay, kern, r32.reshape(1, kmax, NY - 2, NX - 2), w, 0.7, 0.3)
    res = ctx.column_resolution(NX, NY, nlay, kern, w, 0.7, 0.3, rows=True)
    assert ne == res["n_empty"] >= 1
    want = np.einsum("acn,cn->an", res["rows"].reshape(nlay, nlay, NCELL).astype(np.float64), z)
    err = np.abs(x.reshape(nlay, NCELL) - want).max(axis=0) / np.maximum(1.0, np.abs(want).max(axis=0))
    within(f"column_lsq(K z) vs rows @ z, nlay {nlay}", err.max(), 1e-6)
    assert np.abs(want).max() > 0.5                       # (the data do resolve something)


@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("nlay,kmax", [(1, 1), (3, 4), (11, 1), (11, 60), (63, 4), (63, 60)])
def test_bounds_of_a_definite_regulariser(ctx, nlay, kmax, reg):
    """0 <= trace < the cell's number of periods with data (Rm = A^-1 N, N of that rank at most, eigenvalues in [0, 1)), the
    noise std below the posterior std; with damping alone Rm is symmetric and 0 <= Rm_aa < 1.  Each to 1e-6.  (With smoothing Rm is
    not symmetric and Rm_aa leaves [0, 1] in the reference itself: no such bound there.)"""
    kern, w, _ = problem(nlay, kmax, 0)
    got = ctx.column_resolution(NX, NY, nlay, kern, w, *reg, rows=True)
    nper = (w.reshape(kmax, -1) != 0).sum(axis=0)
    assert nper[5] == 1 and nper[3] == 0
    tr = got["trace"].reshape(-1).astype(np.float64)
    on = nper > 0
    within("-min trace", -tr.min(), 1e-6)
    within("max trace / periods with data", (tr[on] / nper[on]).max(), 1.0 + 1e-6)
    assert (tr[on] > 0).all()
    within("max std_noise / std_post", (got["std_noise"].reshape(nlay, -1)[:, on].astype(np.float64)
                                        / got["std_post"].reshape(nlay, -1)[:, on]).max(), 1.0 + 1e-6)
    if reg[0] == 0.0:
        rows = got["rows"].reshape(nlay, nlay, -1).astype(np.float64)
        asym = np.abs(rows - rows.transpose(1, 0, 2)).max(axis=(0, 1)) / np.maximum(1.0, np.abs(rows).max(axis=(0, 1)))
        within("asymmetry of Rm with damping alone", asym.max(), 1e-6)
        within("-min rdiag", -got["rdiag"].min(), 1e-6)
        within("max rdiag", got["rdiag"].max(), 1.0 + 1e-6)


@pytest.mark.parametrize("nlay,kmax", [(7, 9), (63, 60)])
def test_same_factor_as_the_monte_carlo_pass(ctx, nlay, kmax):
    """one Gc/Gs sample on cold columns that carry a known lsen: float32(sqrt(avar)) of the first cold column of each sampled cell
    against std_post for that K, wa, smooth and damp.  Both are dz_column_inverse_factor's sum on dz_column_solve's factor: equal
    bits expected (printed), at most 1 fp32 ulp required."""
    rng = np.random.default_rng(31 + nlay)
    nchain, ntemp = 8, 2
    mc, cells, cobs, amap, wa = grid_problem(ctx, rng, nlay, kmax, nchain, ntemp)
    ncold = nchain // ntemp
    nx = ny = 5
    Kc = trend_kernels(rng, nlay, kmax, mc.ncell)
    lsen = np.ascontiguousarray(np.repeat(Kc[:, :, cells], ncold, axis=2))
    table = np.zeros((nlay, kmax, ny, nx), np.float32)
    table[:, :, 1:-1, 1:-1] = Kc.reshape(nlay, kmax, ny - 2, nx - 2)
    nrm = np.sqrt(((Kc.astype(np.float64) * wa.reshape(kmax, -1).max(axis=1)[None, :, None]) ** 2).sum(axis=1)).max()
    smooth, damp = np.float32(0.12 * nrm), np.float32(0.03 * nrm)
    mc.set_aniso(1, amap, wa, smooth, damp)
    mc.step(curves(rng, mc, cells, cobs, []), 0)
    mc.aniso_step(lsen)
    st = mc.aniso_state()
    assert (st["acnt"] == 1).all() and st["skipped"] == 0
    res = ctx.column_resolution(nx, ny, nlay, table.reshape(nlay, kmax, ny * nx), wa, smooth, damp)
    mc.free()
    assert res["n_empty"] == 1 and res["n_failed"] == 0   # cell (0, 2), where wa is all 0 (the pass keeps the prior's C there)
    keep = cells != 2
    a = np.sqrt(st["avar"][:, ::ncold][:, keep]).astype(np.float32)
    b = np.ascontiguousarray(res["std_post"].reshape(nlay, -1)[:, cells[keep]])
    d = ulps(np.ascontiguousarray(a).ravel(), b.ravel())
    print(f"\n[measured] nlay {nlay} kmax {kmax}: float32(sqrt(avar)) vs std_post, {a.size} values: max {int(d.max())} ulp, "
          f"{int((d == 0).sum())} equal")
    assert a.size == nlay * 7 and (b > 0).all() and d.max() <= 1


def raw_call(ctx, nlay=3, kmax=4, smooth=1.0, damp=0.5, width=True, depz=True):
    nx = ny = 5
    kern = np.zeros(64 * 61 * nx * ny)
    kern[:] = 1.0
    outs = [np.zeros(64 * 9, np.float32) for _ in range(5)]
    z = np.arange(64, dtype=np.float32)
    ne, nf = C.c_int(-1), C.c_int(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = ctx.lib.dazim_column_resolution(ctx._h, nx, ny, nlay, kmax, 0, p(kern), None, C.c_float(smooth), C.c_float(damp),
                                         p(z) if depz else None, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]),
                                         p(outs[4]) if width else None, None, None, C.byref(ne), C.byref(nf))
    return rc, ne.value, nf.value, outs


@pytest.mark.parametrize("bad", ["nlay0", "nlay64", "kmax0", "kmax61", "smooth<0", "damp<0", "both0", "width without depz",
                                 "depz without width"])
def test_refusals(ctx, bad):
    """each refusal returns DAZIM_E_BAD_ARG through the raw entry (buffers large enough for any of the calls) and writes nothing;
    a good call follows"""
    a = {"nlay0": dict(nlay=0), "nlay64": dict(nlay=64), "kmax0": dict(kmax=0), "kmax61": dict(kmax=61), "smooth<0": dict(smooth=-0.1),
         "damp<0": dict(damp=-1e-3), "both0": dict(smooth=0.0, damp=0.0), "width without depz": dict(depz=False),
         "depz without width": dict(width=False)}[bad]
    rc, ne, nf, outs = raw_call(ctx, **a)
    assert rc == dz.DAZIM_E_BAD_ARG and (ne, nf) == (-1, -1) and not any(o.any() for o in outs)
    assert bad.split()[0].rstrip("0123456789<") in ctx.lib.dazim_last_error(ctx._h).decode()
    rc, ne, nf, outs = raw_call(ctx)
    assert rc == 0 and (ne, nf) == (0, 0) and (outs[0][:27] > 0).all() and not outs[0][27:].any()
    rc, ne, nf, outs = raw_call(ctx, width=False, depz=False)
    assert rc == 0 and (outs[0][:27] > 0).all() and not outs[4].any()


def test_a_cell_that_cannot_be_factored_is_nan_and_counted(ctx):
    """a NaN in the kernels of one cell at a period with data: NaN in every output of that cell, counted in n_failed; the same NaN at
    a period without data is not read; the other cells keep their bits"""
    nlay, kmax = 11, 4
    kern, w, depz = problem(nlay, kmax, 0)
    good = ctx.column_resolution(NX, NY, nlay, kern, w, 0.7, 0.3, depz=depz, rows=True)
    wc = w.reshape(kmax, -1)
    cell = 7
    col = (cell // (NX - 2) + 1) * NX + cell % (NX - 2) + 1
    on, off = np.flatnonzero(wc[:, cell] != 0), np.flatnonzero(wc[:, cell] == 0)
    assert len(on) and len(off)
    for p, fails in ((on[0], True), (off[0], False)):
        k2 = kern.copy()
        k2[4, p, col] = np.nan
        got = ctx.column_resolution(NX, NY, nlay, k2, w, 0.7, 0.3, depz=depz, rows=True)
        assert got["n_failed"] == int(fails) and got["n_empty"] == good["n_empty"]
        for k in ref.OUTPUTS:
            g, b = got[k].reshape(-1, NCELL), good[k].reshape(-1, NCELL)
            others = np.arange(NCELL) != cell
            assert np.array_equal(bits(g[:, others]), bits(b[:, others])), k
            assert np.isnan(g[:, cell]).all() if fails else np.array_equal(bits(g[:, cell]), bits(b[:, cell])), k
