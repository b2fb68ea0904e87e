"""-m gpu: dazim_map_posterior: posterior std, resolution matrix and what is derived from it per period, block
and inner cell, from the matrix LSMR is given.

Against numpy.linalg (tests/map_posterior_ref.py) at the sizes the panel width NB = 32 sets (n_g = 1, 31, 32, 33, 65, 135 in
iso-mode; 3, 30, 33, 63, 66, 135 in joint mode, where n_g is a multiple of 3 and 31, 32, 65 cannot occur), kmax 1 and 3, three
regularisers, both tile forms; the arguments that may be left out, host against device arrays, a second call, the column code's
inverse factor, a period that cannot be factored, the refused calls, and the rows of a small synthetic survey."""
import ctypes as C
import functools

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import map_posterior_ref as ref
from tests.bars import within

pytestmark = pytest.mark.gpu

CASES = [(s, False) for s in ref.SHAPES_ISO] + [(s, True) for s in ref.SHAPES_JOINT]
CASE_IDS = [f"{'joint' if az else 'iso'}-{nx}x{ny}" for (nx, ny), az in CASES]
BAR = 1e-6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def n_g(prob):
    return (3 if prob["azim"] else 1) * (prob["nx"] - 2) * (prob["ny"] - 2)


def some_sel(prob):
    ng = n_g(prob)
    return np.unique(np.array([0, ng // 2, ng - 1, ng // 3], np.int32))


@functools.lru_cache(maxsize=None)
def case(nx, ny, azim, reg, kmax, no_reg_period=None):
    prob = ref.problem(nx, ny, kmax, azim, reg[0], reg[1], seed=nx * 100 + ny + 7 * azim + kmax, no_reg_period=no_reg_period)
    for k in ("irow", "icol", "rw"):
        prob[k].setflags(write=False)
    return prob, ref.linalg(prob, some_sel(prob))


def matrix(ctx, prob):
    return ctx.csr_from_coo(prob["m"], prob["n"], prob["irow"], prob["icol"], prob["rw"])


def call(ctx, A, prob, sel=None, width=True):
    return ctx.map_posterior(A, prob["m_data"], prob["nx"], prob["ny"], prob["kmax"], prob["azim"], prob["damp"], sel=sel, width=width)


def same_bits(a, b, keys):
    for k in keys:
        if a[k] is None or b[k] is None:
            continue
        x = a[k].cpu().numpy() if dz._is_torch(a[k]) else a[k]
        y = b[k].cpu().numpy() if dz._is_torch(b[k]) else b[k]
        assert np.array_equal(bits(x), bits(y)), k


@pytest.mark.parametrize("kmax", [1, 3])
@pytest.mark.parametrize("reg", ref.REGS, ids=ref.REG_IDS)
@pytest.mark.parametrize("shape,azim", CASES, ids=CASE_IDS)
def test_equals_numpy_linalg(ctx, shape, azim, reg, kmax):
    """every output within 1e-6 * max(1, max |reference|) of numpy.linalg, with either tile form (their largest mutual difference is
    printed); a second call, torch device arrays, and a call without sel, rows and width give the same bits.
    Measured on an MI355X, largest over the 72 cases and both tile forms: std_post 4.2e-8, std_noise 3.0e-8, rdiag 3.0e-8, rsum
    5.7e-8, width 5.6e-8, leak 3.0e-8, trace 5.5e-8, rows 3.0e-8 (bar 1e-6); the tile forms differ in 2 of the 72 cases, by at most
    7.4e-16."""
    import torch
    prob, want = case(shape[0], shape[1], azim, reg, kmax)
    sel = some_sel(prob)
    A = matrix(ctx, prob)
    assert ctx.stat_or("map_post.nb", ref.NB) == ref.NB
    got = call(ctx, A, prob, sel)
    assert got["n_failed"] == 0 and ctx.stat("map_post.nb") == ref.NB
    tag = f"{'joint' if azim else 'iso'} n_g {n_g(prob)} kmax {kmax}"
    for k, v in ref.worst(got, want).items():
        within(f"map_posterior vs numpy.linalg, {k}, {tag}", v, BAR)
    same_bits(call(ctx, A, prob, sel), got, ref.OUTPUTS)
    dev = call(ctx, A, prob, torch.from_numpy(sel).cuda())
    assert dz._is_torch(dev["std_post"]) and dev["n_failed"] == 0
    same_bits(dev, got, ref.OUTPUTS)
    lean = call(ctx, A, prob, None, width=False)
    assert lean["rows"] is None and lean["width"] is None
    same_bits(lean, got, ("std_post", "std_noise", "rdiag", "rsum", "leak", "trace"))
    assert ctx.stat("map_post.mfma") == 1                  # the default tile form; the plain one:
    ctx.set_option("map_post.mfma", 0)
    try:
        alt = call(ctx, A, prob, sel)
        assert ctx.stat("map_post.mfma") == 0
    finally:
        ctx.set_option("map_post.mfma", 1)
    for k, v in ref.worst(alt, want).items():
        within(f"map_posterior (plain tiles) vs numpy.linalg, {k}, {tag}", v, BAR)
    diff = max(ref.worst(alt, {k: (None if got[k] is None else np.asarray(got[k], np.float64)) for k in ref.OUTPUTS}).values())
    print(f"\n[measured] {tag}: largest difference between the tile forms {diff:.3e}")
    A.free()


@pytest.mark.parametrize("ncell", [(3, 3), (9, 5), (11, 9)], ids=["n1", "n21", "n63"])
def test_same_numbers_as_the_column_codes_inverse_factor(ctx, ncell):
    """iso, one period, damping alone, at most 60 data rows and 63 unknowns: the same dense normal matrix through
    dazim_column_resolution (K = the data rows, one cell, smooth 0), whose C_aa is dz_column_inverse_factor's sum.  The two inverses
    differ in the order of their sums only: std_post within 1 fp32 ulp, the number of equal values printed (measured on an MI355X:
    0 ulp, all 1 + 21 + 63 values equal)."""
    nx, ny = ncell
    prob = ref.problem(nx, ny, 1, False, 0.0, 0.4, seed=3, rays_per_period=min(60, 2 * (nx - 2) * (ny - 2) + 3))
    ng, nd = n_g(prob), prob["m_data"]
    A = matrix(ctx, prob)
    got = call(ctx, A, prob)
    A.free()
    dense = np.zeros((nd, ng))
    dense[prob["irow"] - 1, prob["icol"] - 1] = prob["rw"]
    kern = np.zeros((ng, nd, 9))
    kern[:, :, 4] = dense.T
    col = ctx.column_resolution(3, 3, ng, kern, None, 0.0, prob["damp"])
    assert col["n_failed"] == 0 and col["n_empty"] == 0
    a, b = got["std_post"].reshape(-1), col["std_post"].reshape(-1)
    d = np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))
    print(f"\n[measured] n_g {ng}: std_post against the column code, {a.size} values: max {int(d.max())} ulp, {int((d == 0).sum())} equal")
    assert d.max() <= 1


def test_a_period_that_cannot_be_factored_is_nan_and_counted(ctx):
    """smoothing alone, no regularisation rows for period 1, and the map's last cell without rays: NaN in every output of period 1
    only, n_failed 1, the other periods within the bar"""
    prob, want = case(9, 5, True, (0.8, 0.0), 3, no_reg_period=1)
    assert want["n_failed"] == 1
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, some_sel(prob))
    A.free()
    assert got["n_failed"] == 1
    for k in ref.OUTPUTS:
        a = np.moveaxis(got[k], 0 if k == "rows" else 1, 0)
        assert np.isnan(a[1]).all() and np.isfinite(a[[0, 2]]).all(), k
    for k, v in ref.worst(got, want).items():
        within(f"map_posterior beside a failed period, {k}", v, BAR)


SENTINEL = np.float32(-7.5)


def raw_call(ctx, A, prob, m_data=None, nx=None, azim=None, missing=None, leak=None, sel=None, rows=False, damp=None):
    nblk = 3 if prob["azim"] else 1
    ng = n_g(prob)
    outs = {k: np.full(nblk * prob["kmax"] * ng + 8, SENTINEL) for k in ("std_post", "std_noise", "rdiag", "rsum", "width", "leak")}
    outs["rows"] = np.full(prob["kmax"] * 4 * ng, SENTINEL)
    outs["trace"] = np.full(nblk * prob["kmax"], SENTINEL)
    p = lambda k: None if k == missing else C.c_void_p(outs[k].ctypes.data)
    use_leak = prob["azim"] if leak is None else leak
    sel = None if sel is None else np.ascontiguousarray(sel, np.int32)
    nf = C.c_int(-1)
    rc = ctx.lib.dazim_map_posterior(ctx._h, A._h, C.c_int64(prob["m_data"] if m_data is None else m_data), prob["nx"] if nx is None else nx,
                                     prob["ny"], prob["kmax"], int(prob["azim"] if azim is None else azim),
                                     C.c_float(prob["damp"] if damp is None else damp), p("std_post"), p("std_noise"), p("rdiag"), p("rsum"),
                                     p("width"), p("leak") if use_leak else None, 0 if sel is None else len(sel),
                                     None if sel is None else C.c_void_p(sel.ctypes.data), p("rows") if rows else None, p("trace"), C.byref(nf))
    return rc, nf.value, outs


REFUSALS = {"m_data<0": dict(m_data=-1), "m_data>m": dict(m_data=10 ** 6), "n": dict(nx=8), "no std_post": dict(missing="std_post"),
            "no std_noise": dict(missing="std_noise"), "no rdiag": dict(missing="rdiag"), "no rsum": dict(missing="rsum"),
            "sel<0": dict(sel=[0, -1]), "sel>=n_g": dict(sel=[1, 10 ** 4]), "rows without sel": dict(rows=True), "damp<0": dict(damp=-0.1)}


@pytest.mark.parametrize("bad", sorted(REFUSALS))
def test_refusals(ctx, bad):
    """each refused call returns DAZIM_E_BAD_ARG through the raw entry and writes nothing; a good call follows"""
    prob, _ = case(9, 5, True, (0.7, 0.3), 3)
    A = matrix(ctx, prob)
    rc, nf, outs = raw_call(ctx, A, prob, **REFUSALS[bad])
    assert rc == dz.DAZIM_E_BAD_ARG and nf == -1 and all((o == SENTINEL).all() for o in outs.values()), bad
    rc, nf, outs = raw_call(ctx, A, prob, sel=[2, 5], rows=True)
    assert rc == 0 and nf == 0 and (outs["std_post"][:3 * 3 * 21] > 0).all() and (outs["std_post"][3 * 3 * 21:] == SENTINEL).all()
    assert (outs["rows"][:3 * 2 * 63] != SENTINEL).all() and (outs["rows"][3 * 2 * 63:] == SENTINEL).all()
    A.free()


def test_leak_without_azim_is_refused(ctx):
    prob, _ = case(9, 5, False, (0.7, 0.3), 3)
    A = matrix(ctx, prob)
    rc, nf, outs = raw_call(ctx, A, prob, leak=True)
    assert rc == dz.DAZIM_E_BAD_ARG and nf == -1 and all((o == SENTINEL).all() for o in outs.values())
    assert "leak" in ctx.lib.dazim_last_error(ctx._h).decode()
    rc, nf, outs = raw_call(ctx, A, prob)
    assert rc == 0 and nf == 0 and (outs["leak"] == SENTINEL).all()
    A.free()


@pytest.mark.parametrize("where", ["data row", "regularisation row"])
def test_a_row_in_two_periods_is_refused(ctx, where):
    """found on the device: one more entry, in another period's columns, on a data row or on a regularisation row"""
    prob, _ = case(9, 5, True, (0.7, 0.3), 3)
    row = 1 if where == "data row" else prob["m"]
    mine = prob["icol"][prob["irow"] == row]
    ncell, kmax = 21, 3
    p = ((mine[0] - 1) % (kmax * ncell)) // ncell
    extra = 2 * kmax * ncell + ((p + 1) % kmax) * ncell + 5 + 1     # a2 block, the next period, cell 5 (1-based column)
    assert extra not in mine
    bad = dict(prob, irow=np.append(prob["irow"], row).astype(np.int32), icol=np.append(prob["icol"], extra).astype(np.int32),
               rw=np.append(prob["rw"], np.float32(0.25)))
    A = matrix(ctx, bad)
    rc, nf, outs = raw_call(ctx, A, bad)
    assert rc == dz.DAZIM_E_BAD_ARG and nf == -1 and all((o == SENTINEL).all() for o in outs.values())
    assert "two periods" in ctx.lib.dazim_last_error(ctx._h).decode()
    A.free()


def test_rows_of_a_synthetic_survey(ctx):
    """real rows: the small synthetic of tests/test_phase_maps_gpu.py (fewer stations), rays_build_G_maps with azim, weighted and
    regularised as the maps program does; the triplets taken back through to_coo for the reference.  Measured on an MI355X (480
    rays, n_g 297, cond(A_g) 3.2e2): largest over the outputs 3.8e-8 (width); median std_post of c 0.155 km/s, median leak of c 0.42."""
    from tests.test_phase_maps_gpu import DV, GOXD, GOZD, survey, true_maps
    nx, ny, kmax, damp = 13, 11, 2, 0.01
    scx, scz, per, ray_f, rx, rz = survey(nx, ny, kmax, 10, None, seed=21)
    pv_true, pv, _ = true_maps(nx, ny, kmax, True)
    fields = ctx.fmm_batch(nx, ny, GOXD, GOZD, DV, DV, pv_true, scx, scz, per)
    Gt, tobs, _ = ctx.rays_build_G_maps(nx, ny, GOXD, GOZD, DV, DV, fields, scx, scz, per, ray_f, rx, rz, azim=True)
    tobs = tobs.copy()
    Gt.free()
    fields = ctx.fmm_batch(nx, ny, GOXD, GOZD, DV, DV, pv, scx, scz, per)
    G, tp, _ = ctx.rays_build_G_maps(nx, ny, GOXD, GOZD, DV, DV, fields, scx, scz, per, ray_f, rx, rz, azim=True)
    m_data = G.m
    ctx.weight_data(G, tobs, tp.copy())
    G.append_laplacian2d(nx, ny, np.array([2.0] * kmax + [4.0] * 2 * kmax, np.float32))
    irow, icol, rw = G.to_coo()
    prob = dict(nx=nx, ny=ny, kmax=kmax, azim=True, damp=float(np.float32(damp)), m=G.m, m_data=m_data, n=G.n, irow=irow, icol=icol, rw=rw)
    sel = some_sel(prob)
    got = call(ctx, G, prob, sel)
    G.free()
    want = ref.linalg(prob, sel)
    conds = [np.linalg.cond(ref.normal_matrix(prob, D, L)) for D, L, _ in ref.groups(prob)]
    print(f"\n[measured] synthetic survey: {m_data} rays, n_g {n_g(prob)}, cond(A_g) {max(conds):.2e}, median std_post(c) "
          f"{np.median(got['std_post'][0]):.4f} km/s, median leak(c) {np.median(got['leak'][0]):.3f}")
    assert got["n_failed"] == want["n_failed"] == 0
    for k, v in ref.worst(got, want).items():
        within(f"map_posterior vs numpy.linalg on a synthetic survey, {k}", v, BAR)
