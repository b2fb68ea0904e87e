"""-m gpu: dazim_column_lsq_radial and dazim_column_resolution_radial: Vsv and Vsh updates per inner cell from
Rayleigh and Love kernels, tied by a prior towards isotropy, and their posterior.

Against the fp64 restatement (tests/column_radial_ref.py: the stacked system through numpy.linalg.lstsq, the posterior through
numpy.linalg.inv), against dazim_column_lsq block by block without coupling, under the swap of the two blocks, against the solve
itself (noise-free data: x = Rm z), the refused calls and the special cells.  nx = 7, ny = 6: 20 cells; radial_problem's cell 3 has
no data in either block, cell 5 a single period, cell 7 Love data only.  nlay 1, 2, 32, 33, 63: N = 2, 4, 64 (one wavefront wide),
66 (the first size on 128 lanes) and 126 (the largest LDS request, 96 216 bytes with kv + kh = 60).
Measured on an MI355X, largest over the cases: x against lstsq 5.8e-8 (bar 1e-6); each block against dazim_column_lsq without
coupling 0 ulp; x against rows @ z 8.9e-8; std 5.8e-8, rdiag 5.7e-8, rsum 5.9e-8, trace 5.9e-8, rows 6.1e-8 (bar 1e-6), cov_vh 5.7e-8
(bar 1.2e-7), cross 1.9e-6 (bar 3.9e-6); the halves under the swap x 1.5e-11, std 0, cross 6.0e-8."""
import ctypes as C
import functools

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import column_radial_ref as ref
from tests.bars import within
from tests.test_column_mc_aniso_gpu import ulps

pytestmark = pytest.mark.gpu

NX, NY = 7, 6
NCELL = (NX - 2) * (NY - 2)
REGS = [(0.7, 0.3), (0.0, 0.5), (0.8, 0.0)]
REG_IDS = ["smooth+damp", "damp", "smooth"]
NLAYS = [1, 2, 32, 33, 63]
PERIODS = [(1, 0), (0, 1), (1, 1), (16, 7), (30, 30), (60, 0), (0, 60)]
COUPLES = [0.0, 0.7, 50.0]
# cov_vh and cross against numpy.linalg: twice the largest of the 315 cases measured on an MI355X.  cov_vh
# 5.7e-8, which is fp32 rounding (2^-24 = 6.0e-8 of max(1, max |reference|)).  cross 1.9e-6 (nlay 63, 60 Love periods, smoothing
# alone, couple 50; above 1.2e-7 in 5 of the 315 cases, all smoothing alone with couple 50): a ratio whose denominator, the row's
# sum of |Rm_ac|, is small for a knot the data hardly reach, so that the 1e-9 which Rm = I - C P2 loses against |C| |P2| = 7e3 * 2.5e3
# shows; the rows themselves are within 6.1e-8.
BAR_COV_VH, BAR_CROSS = 1.2e-7, 3.9e-6


@functools.lru_cache(maxsize=None)
def problem(nlay, kv, kh):
    p = ref.radial_problem(NX, NY, nlay, kv, kh, seed=nlay * 1000 + kv * 10 + kh)
    for a in p:
        if a is not None:
            a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def solution(nlay, kv, kh, reg, couple):
    kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = problem(nlay, kv, kh)
    return ref.per_cell_solve(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0, *reg, couple)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def on_device(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def cell_error(x, xn):
    """per cell max |x - xn| / max(1, max |xn|), x and xn [..][ncell]"""
    x, xn = np.asarray(x, np.float64).reshape(-1, NCELL), np.asarray(xn, np.float64).reshape(-1, NCELL)
    return np.abs(x - xn).max(axis=0) / np.maximum(1.0, np.abs(xn).max(axis=0))


@pytest.mark.parametrize("couple", COUPLES)
@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("kv,kh", PERIODS)
@pytest.mark.parametrize("nlay", NLAYS)
def test_equals_numpy_lstsq(ctx, nlay, kv, kh, reg, couple):
    """x within 1e-6 * max(1, max |x_np|) of the stacked lstsq in every cell, 0 exactly in the cell without data (counted in n_empty),
    the RMS statistics within 1e-5 relative; device (torch) arrays give the bits of host arrays"""
    kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = problem(nlay, kv, kh)
    xn, nen, stn = solution(nlay, kv, kh, reg, couple)
    x, ne, st = ctx.column_lsq_radial(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0, *reg, couple)
    assert x.shape == (2, nlay, NY - 2, NX - 2) and x.dtype == np.float32 and st.shape == (kv + kh, 2)
    assert ne == nen >= 1 and not bits(x).reshape(2 * nlay, NCELL)[:, 3].any()
    within(f"column_lsq_radial vs lstsq, nlay {nlay} kv {kv} kh {kh} couple {couple}", cell_error(x, xn).max(), 1e-6)
    assert np.allclose(st, stn, rtol=1e-5, atol=0), np.abs(st - stn).max()
    xd, ned, std = ctx.column_lsq_radial(NX, NY, nlay, *on_device(kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0), *reg, couple)
    assert ned == ne and np.array_equal(bits(xd.cpu().numpy()), bits(x)) and np.array_equal(bits(std), bits(st))


@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("kv,kh", PERIODS)
@pytest.mark.parametrize("nlay", NLAYS)
def test_without_coupling_each_block_is_column_lsq(ctx, nlay, kv, kh, reg):
    """couple = 0, whatever d0 is: each block within one fp32 ulp of dazim_column_lsq on that block alone (the same operations in the
    same order: equal bits expected, printed), a block without data exactly 0"""
    kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = problem(nlay, kv, kh)
    x, ne, st = ctx.column_lsq_radial(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0, *reg, 0.0)
    off = 0
    for blk, (kern, rhs, w) in enumerate(((kern_v, rhs_v, w_v), (kern_h, rhs_h, w_h))):
        if kern is None:
            assert not bits(x[blk]).any()
            continue
        xb, _, stb = ctx.column_lsq(NX, NY, nlay, kern, rhs[None], w, *reg)
        d = ulps(np.ascontiguousarray(x[blk]).ravel(), np.ascontiguousarray(xb[0]).ravel())
        print(f"\n[measured] block {blk} vs column_lsq, nlay {nlay} kv {kv} kh {kh}: max {int(d.max())} ulp, {int((d == 0).sum())} of {d.size} equal")
        assert d.max() <= 1
        none = ~(w.reshape(kern.shape[1], -1) != 0).any(axis=0)
        assert none[3] and not bits(x[blk]).reshape(nlay, NCELL)[:, none].any()
        assert np.allclose(st[off:off + kern.shape[1]], stb[0], rtol=1e-6, atol=0)
        off += kern.shape[1]


@pytest.mark.parametrize("couple", COUPLES)
@pytest.mark.parametrize("kv,kh", [(1, 0), (1, 1), (16, 7), (60, 0)])
@pytest.mark.parametrize("nlay", NLAYS)
def test_block_symmetry(ctx, nlay, kv, kh, couple):
    """swap (kern, rhs, w) between the two blocks and negate d0: the two halves of x swap, within 1e-6 * max(1, max |x|) per cell, and so
    do the halves of the posterior; cov_vh stays"""
    kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = problem(nlay, kv, kh)
    x, ne, st = ctx.column_lsq_radial(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0, 0.7, 0.3, couple)
    y, ney, sty = ctx.column_lsq_radial(NX, NY, nlay, kern_h, kern_v, rhs_h, rhs_v, w_h, w_v, -d0, 0.7, 0.3, couple)
    assert ne == ney
    within(f"halves of x under the swap, nlay {nlay} kv {kv} kh {kh} couple {couple}", cell_error(y[::-1], x).max(), 1e-6)
    assert np.allclose(np.concatenate([sty[kh:], sty[:kh]]), st, rtol=1e-5, atol=0)
    a = ctx.column_resolution_radial(NX, NY, nlay, kern_v, kern_h, w_v, w_h, 0.7, 0.3, couple)
    b = ctx.column_resolution_radial(NX, NY, nlay, kern_h, kern_v, w_h, w_v, 0.7, 0.3, couple)
    for k in ref.PER_KNOT + ("trace",):
        within(f"halves of {k} under the swap, nlay {nlay}", cell_error(b[k][::-1], a[k]).max(), 1e-6)
    within(f"cov_vh under the swap, nlay {nlay}", cell_error(b["cov_vh"], a["cov_vh"]).max(), 1e-6)


@functools.lru_cache(maxsize=None)
def posterior(nlay, kv, kh, reg, couple):
    kern_v, kern_h, _, _, w_v, w_h, _ = problem(nlay, kv, kh)
    return ref.per_cell_res(ref.linalg, NX, NY, nlay, kern_v, kern_h, w_v, w_h, *reg, couple)


@pytest.mark.parametrize("couple", COUPLES)
@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("kv,kh", PERIODS)
@pytest.mark.parametrize("nlay", NLAYS)
def test_resolution_equals_numpy_linalg(ctx, nlay, kv, kh, reg, couple):
    """std, rdiag, rsum, trace and rows within 1e-6 * max(1, max |reference|) of numpy.linalg per cell (the bar of
    test_column_resolution_gpu), cov_vh and cross within their own bars; the cell without data 0 in every output and counted; torch
    device arrays give the bits of host arrays; leaving out rows changes no bit of the rest.  cov_vh^2 <= std_v^2 std_h^2 always (C is
    definite); 0 <= rdiag <= 1 within rounding where P2 is a multiple of I (damping alone, no coupling): Rm = A^-1 N is then
    symmetric with eigenvalues in [0, 1).  With smoothing or coupling Rm is not symmetric and Rm_aa leaves [0, 1] in the fp64
    reference itself (nlay 11, kv = kh = 4: -1.02 with smoothing alone, -0.041 with damping and couple = 50), as the note in
    test_column_resolution_gpu says of the isotropic problem: no such bound there."""
    kern_v, kern_h, _, _, w_v, w_h, _ = problem(nlay, kv, kh)
    want = posterior(nlay, kv, kh, reg, couple)
    got = ctx.column_resolution_radial(NX, NY, nlay, kern_v, kern_h, w_v, w_h, *reg, couple, rows=True)
    assert got["n_empty"] == want["n_empty"] >= 1 and got["n_failed"] == 0
    assert got["rows"].shape == (2 * nlay, 2 * nlay, NY - 2, NX - 2) and got["trace"].shape == (2, NY - 2, NX - 2)
    assert got["std"].shape == (2, nlay, NY - 2, NX - 2) and got["cov_vh"].shape == (nlay, NY - 2, NX - 2)
    for k in ref.OUTPUTS:
        assert got[k].dtype == np.float32 and not bits(got[k]).reshape(-1, NCELL)[:, 3].any(), k
    worst = ref.worst(got, want)
    for k in ("std", "rdiag", "rsum", "trace", "rows"):
        within(f"column_resolution_radial vs numpy.linalg, {k}, nlay {nlay} kv {kv} kh {kh} couple {couple}", worst[k], 1e-6)
    within(f"column_resolution_radial vs numpy.linalg, cov_vh, nlay {nlay} kv {kv} kh {kh} couple {couple}", worst["cov_vh"], BAR_COV_VH)
    within(f"column_resolution_radial vs numpy.linalg, cross, nlay {nlay} kv {kv} kh {kh} couple {couple}", worst["cross"], BAR_CROSS)
    sd = got["std"].astype(np.float64)
    within("max cov_vh^2 / (std_v^2 std_h^2)", (got["cov_vh"].astype(np.float64) ** 2 / np.maximum(sd[0] ** 2 * sd[1] ** 2, 1e-300)).max(), 1.0 + 1e-6)
    if reg[0] == 0.0 and couple == 0.0:
        within("-min rdiag", -got["rdiag"].min(), 1e-6)
        within("max rdiag", got["rdiag"].max(), 1.0 + 1e-6)
    dev = ctx.column_resolution_radial(NX, NY, nlay, *on_device(kern_v, kern_h, w_v, w_h), *reg, couple, rows=True)
    assert (dev["n_empty"], dev["n_failed"]) == (got["n_empty"], 0)
    for k in ref.OUTPUTS:
        assert np.array_equal(bits(dev[k].cpu().numpy()), bits(got[k])), k
    lean = ctx.column_resolution_radial(NX, NY, nlay, kern_v, kern_h, w_v, w_h, *reg, couple)
    assert lean["rows"] is None
    for k in ref.PER_KNOT + ("cov_vh", "trace"):
        assert np.array_equal(bits(lean[k]), bits(got[k])), k


@pytest.mark.parametrize("couple", COUPLES)
@pytest.mark.parametrize("nlay", NLAYS)
def test_it_is_the_solves_resolution(ctx, nlay, couple):
    """integer K (|K| <= 8), integer z (|z| <= 4), weights that are powers of two: r = K z is exact in fp32, so with d0 = 0
    dazim_column_lsq_radial's x for it is Rm z: x against rows @ z (rows widened to fp64) within 1e-6 * max(1, max |rows @ z|) per cell"""
    kv, kh = 12, 9
    rng = np.random.default_rng(77 + nlay)
    kern = [rng.integers(-8, 9, (nlay, k, NX * NY)).astype(np.float64) for k in (kv, kh)]
    z = rng.integers(-4, 5, (2, nlay, NCELL)).astype(np.float64)
    w, r = [], []
    for blk, k in enumerate((kv, kh)):
        wb = (2.0 ** rng.integers(-1, 2, (k, NCELL))).astype(np.float32)
        wb[rng.random((k, NCELL)) < 0.25] = 0.0
        wb[:, 3] = 0.0
        Kc = kern[blk].reshape(nlay, k, NY, NX)[:, :, 1:-1, 1:-1].reshape(nlay, k, NCELL)
        rb = np.einsum("lpc,lc->pc", Kc, z[blk])
        assert np.array_equal(rb.astype(np.float32).astype(np.float64), rb)
        w.append(wb.reshape(k, NY - 2, NX - 2))
        r.append(rb.astype(np.float32).reshape(k, NY - 2, NX - 2))
    x, ne, _ = ctx.column_lsq_radial(NX, NY, nlay, kern[0], kern[1], r[0], r[1], w[0], w[1], None, 0.7, 0.3, couple)
    res = ctx.column_resolution_radial(NX, NY, nlay, kern[0], kern[1], w[0], w[1], 0.7, 0.3, couple, rows=True)
    assert ne == res["n_empty"] >= 1 and res["n_failed"] == 0
    want = np.einsum("acn,cn->an", res["rows"].reshape(2 * nlay, 2 * nlay, NCELL).astype(np.float64), z.reshape(2 * nlay, NCELL))
    within(f"column_lsq_radial(K z) vs rows @ z, nlay {nlay} couple {couple}", cell_error(x, want).max(), 1e-6)
    assert np.abs(want).max() > 0.5                       # (the data do resolve something)


def test_a_cell_with_love_data_only_follows_through_the_coupling(ctx):
    """cell 7 has no Rayleigh data: without coupling its Vsv update is exactly 0, with coupling it is not, and the cell is solved,
    not counted as empty"""
    nlay, kv, kh = 11, 16, 7
    kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = problem(nlay, kv, kh)
    assert not w_v.reshape(kv, -1)[:, 7].any() and w_h.reshape(kh, -1)[:, 7].any()
    x0, ne0, _ = ctx.column_lsq_radial(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, None, 0.7, 0.3, 0.0)
    x1, ne1, _ = ctx.column_lsq_radial(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, None, 0.7, 0.3, 5.0)
    assert ne0 == ne1 == 1
    assert not bits(x0[0]).reshape(nlay, NCELL)[:, 7].any() and x0[1].reshape(nlay, NCELL)[:, 7].any()
    assert np.abs(x1[0].reshape(nlay, NCELL)[:, 7]).max() > 1e-3


def test_without_weights_and_d0_is_ones_and_zeros(ctx):
    nlay, kv, kh = 5, 7, 3
    kern_v, kern_h, rhs_v, rhs_h, _, _, _ = problem(nlay, kv, kh)
    ones = [np.ones((k, NY - 2, NX - 2), np.float32) for k in (kv, kh)]
    zero = np.zeros((nlay, NY - 2, NX - 2), np.float32)
    x, ne, st = ctx.column_lsq_radial(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, None, None, None, 0.5, 0.1, 0.7)
    x1, ne1, st1 = ctx.column_lsq_radial(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, *ones, zero, 0.5, 0.1, 0.7)
    assert ne == ne1 == 0 and np.array_equal(bits(x), bits(x1)) and np.array_equal(bits(st), bits(st1))
    a = ctx.column_resolution_radial(NX, NY, nlay, kern_v, kern_h, None, None, 0.5, 0.1, 0.7, rows=True)
    b = ctx.column_resolution_radial(NX, NY, nlay, kern_v, kern_h, *ones, 0.5, 0.1, 0.7, rows=True)
    for k in ref.OUTPUTS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


BAD = {"nlay0": dict(nlay=0), "nlay64": dict(nlay=64), "kv<0": dict(kv=-1), "kh<0": dict(kh=-1), "kv+kh=0": dict(kv=0, kh=0, kern_v=False, kern_h=False),
       "kv+kh=61": dict(kv=30, kh=31), "smooth<0": dict(smooth=-0.1), "damp<0": dict(damp=-1e-3), "couple<0": dict(couple=-0.5),
       "both0": dict(smooth=0.0, damp=0.0), "kern_v missing": dict(kern_v=False), "kern_h missing": dict(kern_h=False),
       "kern_v with kv=0": dict(kv=0), "output missing": dict(out=False)}


def raw_calls(ctx, nlay=3, kv=4, kh=2, smooth=1.0, damp=0.5, couple=0.7, kern_v=True, kern_h=True, out=True):
    """both raw entries on buffers large enough for any of the calls: (rc of the solve, rc of the resolution, the outputs, counters)"""
    nx = ny = 5
    kern = np.ones(64 * 61 * nx * ny)
    rhs = np.ones(61 * 9, np.float32)
    outs = [np.zeros(2 * 64 * 9, np.float32) for _ in range(6)]
    cnt = [C.c_int(-1) for _ in range(3)]
    p = lambda a: C.c_void_p(a.ctypes.data)
    kvp, khp = p(kern) if kern_v else None, p(kern) if kern_h else None
    f = lambda v: C.c_float(v)
    rc1 = ctx.lib.dazim_column_lsq_radial(ctx._h, nx, ny, nlay, kv, kvp, kh, khp, p(rhs), p(rhs), None, None, None, f(smooth), f(damp), f(couple),
                                          p(outs[0]) if out else None, C.byref(cnt[0]), None)
    rc2 = ctx.lib.dazim_column_resolution_radial(ctx._h, nx, ny, nlay, kv, kvp, kh, khp, None, None, f(smooth), f(damp), f(couple),
                                                 p(outs[1]) if out else None, p(outs[2]), p(outs[3]), p(outs[4]), p(outs[5]), None, None,
                                                 C.byref(cnt[1]), C.byref(cnt[2]))
    return rc1, rc2, outs, [c.value for c in cnt]


@pytest.mark.parametrize("bad", list(BAD))
def test_refusals(ctx, bad):
    """each refusal returns DAZIM_E_BAD_ARG from both raw entries and writes nothing; a good call follows"""
    rc1, rc2, outs, cnt = raw_calls(ctx, **BAD[bad])
    assert rc1 == rc2 == dz.DAZIM_E_BAD_ARG and cnt == [-1, -1, -1] and not any(o.any() for o in outs)
    assert "dazim_column_resolution_radial" in ctx.lib.dazim_last_error(ctx._h).decode()
    rc1, rc2, outs, cnt = raw_calls(ctx)
    assert rc1 == rc2 == 0 and cnt == [0, 0, 0] and outs[0][:54].any() and (outs[1][:54] > 0).all() and not outs[1][54:].any()


def test_a_cell_that_cannot_be_factored_is_nan_and_counted(ctx):
    """a NaN in the Love kernels of one cell at a period with data: NaN in every resolution output of that cell, counted in n_failed;
    the same NaN at a period without data is not read; the other cells keep their bits"""
    nlay, kv, kh = 11, 4, 4
    kern_v, kern_h, _, _, w_v, w_h, _ = problem(nlay, kv, kh)
    good = ctx.column_resolution_radial(NX, NY, nlay, kern_v, kern_h, w_v, w_h, 0.7, 0.3, 0.7, rows=True)
    wc = w_h.reshape(kh, -1)
    cell = next(c for c in range(8, NCELL) if 0 < (wc[:, c] != 0).sum() < kh)
    col = (cell // (NX - 2) + 1) * NX + cell % (NX - 2) + 1
    on, off = np.flatnonzero(wc[:, cell] != 0), np.flatnonzero(wc[:, cell] == 0)
    assert len(on) and len(off)
    for p, fails in ((on[0], True), (off[0], False)):
        k2 = kern_h.copy()
        k2[4, p, col] = np.nan
        got = ctx.column_resolution_radial(NX, NY, nlay, kern_v, k2, w_v, w_h, 0.7, 0.3, 0.7, rows=True)
        assert got["n_failed"] == int(fails) and got["n_empty"] == good["n_empty"]
        for k in ref.OUTPUTS:
            g, b = got[k].reshape(-1, NCELL), good[k].reshape(-1, NCELL)
            others = np.arange(NCELL) != cell
            assert np.array_equal(bits(g[:, others]), bits(b[:, others])), k
            assert np.isnan(g[:, cell]).all() if fails else np.array_equal(bits(g[:, cell]), bits(b[:, cell])), k
