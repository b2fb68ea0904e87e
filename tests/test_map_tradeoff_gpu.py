"""-m gpu: dazim_map_tradeoff: the maps' linearised step solved exactly, per period, at every point of a sweep
over regularisation strengths, with chi2, the regularisation norms, log-determinants, degrees of freedom, GCV and the evidence.

Against numpy.linalg (tests/map_tradeoff_ref.py) on map_posterior_ref's problems (n_g = 1, 31, 32, 33, 65, 135 in iso-mode; 3, 30, 33,
63, 66, 135 with azim: both sides of the panel width 32 and of the 64-tile) at kmax 3, the two n_g = 33 shapes at kmax 1 too, three
regularisers, both tile forms; bit equality of a second call, a device right-hand side, every point alone, the sweep reversed and the
calls with dof or evidence off; one Gram pass per period whatever K; dazim_map_posterior's trace; a (point, period) that cannot be
factored; a prior that is not positive definite; a period without data; the refused calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import map_posterior_ref as mref
from tests import map_tradeoff_ref as ref
from tests import model_tradeoff_ref as tref
from tests.bars import within

pytestmark = pytest.mark.gpu

CASES = [(s, False, 3) for s in mref.SHAPES_ISO] + [(s, True, 3) for s in mref.SHAPES_JOINT] + [((13, 5), False, 1), ((13, 3), True, 1)]
CASE_IDS = [f"{'azim' if az else 'iso'}-{nx}x{ny}-kmax{kmax}" for (nx, ny), az, kmax in CASES]
BAR = 1e-6   # the bar of tests/test_map_posterior_gpu.py for these dense kernels


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def case(shape, azim, reg, kmax):
    """the problem and sweep tests/test_map_tradeoff_ref_cpu.py bounds the condition of, and its reference"""
    prob = ref.problem(shape[0], shape[1], kmax, azim, reg)
    scale, damp = ref.sweep(prob)
    for a in (prob["irow"], prob["icol"], prob["rw"], prob["b"], scale, damp):
        a.setflags(write=False)
    return prob, scale, damp, ref.linalg(prob, scale, damp)


def matrix(ctx, prob):
    return ctx.csr_from_coo(prob["m"], prob["n"], prob["irow"], prob["icol"], prob["rw"])


def call(ctx, A, prob, scale, damp, b=None, **kw):
    kw.setdefault("x", True)
    return ctx.map_tradeoff(A, prob["m_data"], prob["b"] if b is None else b, prob["nx"], prob["ny"], prob["kmax"], prob["azim"], scale, damp, **kw)


def same_bits(a, b, keys=ref.OUTPUTS, ia=slice(None), ib=slice(None)):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(bits(a[k][ia]), bits(b[k][ib])), k
    assert np.array_equal(a["n_failed"][ia], b["n_failed"][ib]) and np.array_equal(a["mdata_p"], b["mdata_p"])


def picks_of(out):
    reg2sum = out["reg2"].sum(axis=2)
    return [tref.pick(out["chi2"][:, p], reg2sum[:, p], out["gcv"][:, p], out["logev"][:, p]) for p in range(out["chi2"].shape[1])]


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("shape,azim,kmax", CASES, ids=CASE_IDS)
def test_equals_numpy_linalg_and_bits_hold(ctx, shape, azim, kmax, reg):
    """every output within 1e-6 * max(1, max |reference|) of numpy.linalg, with either tile form (the largest value is printed), the
    totals too, the picks those of the NumPy rules; the same bits from a second call, a device b, the sweep reversed (which a clobbered
    D_p would not survive), every point alone, and from the calls without dof or without the evidence in the outputs that remain;
    map_trade.grams is kmax for the whole sweep and for one point.
    Measured on an MI355X, largest over the 42 cases and both tile forms: 5.1e-08 (bar 1e-6)."""
    import torch
    prob, scale, damp, want = case(shape, azim, reg, kmax)
    K = len(damp)
    ng = (3 if azim else 1) * (shape[0] - 2) * (shape[1] - 2)
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, scale, damp)
    assert not got["n_failed"].any() and ctx.stat("map_trade.ng") == ng and ctx.stat("map_trade.points") == K
    assert ctx.stat("map_trade.grams") == kmax and np.array_equal(got["mdata_p"], want["mdata_p"])
    tag = f"{'azim' if azim else 'iso'} n_g {ng} kmax {kmax}"
    big = 0.0
    for k, v in ref.worst(got, want).items():
        big = max(big, v)
        within(f"map_tradeoff vs numpy.linalg, {k}, {tag}", v, BAR)
    for k, v in tref.worst(got["total"], ref.totals(want), ref.TOTALS).items():
        big = max(big, v)
        within(f"map_tradeoff totals vs numpy, {k}, {tag}", v, BAR)
    assert got["pick"] == picks_of(got)
    tot = got["total"]
    assert got["pick_total"] == tref.pick(tot["chi2"], tot["reg2sum"], tot["gcv"], tot["logev"])
    same_bits(call(ctx, A, prob, scale, damp), got)
    same_bits(call(ctx, A, prob, scale, damp, b=torch.from_numpy(prob["b"].copy()).cuda()), got)
    same_bits(call(ctx, A, prob, scale[::-1].copy(), damp[::-1].copy()), got, ib=slice(None, None, -1))
    for k in range(K):
        same_bits(call(ctx, A, prob, scale[k:k + 1], damp[k:k + 1]), got, ib=slice(k, k + 1))
        assert ctx.stat("map_trade.grams") == kmax and ctx.stat("map_trade.points") == 1
    nodof = call(ctx, A, prob, scale, damp, dof=False)
    assert nodof["dof"] is None and nodof["gcv"] is None and nodof["total"]["gcv"] is None
    same_bits(nodof, got, ("chi2", "reg2", "xnorm2", "logdet_a", "logdet_p", "logev", "x"))
    noev = call(ctx, A, prob, scale, damp, evidence=False, x=False)
    assert noev["logdet_p"] is None and noev["logev"] is None and noev["x"] is None
    same_bits(noev, got, ("chi2", "reg2", "xnorm2", "logdet_a", "dof", "gcv"))
    ctx.set_option("map_post.mfma", 0)                     # the plain tile form
    try:
        alt = call(ctx, A, prob, scale, damp)
    finally:
        ctx.set_option("map_post.mfma", 1)
    for k, v in ref.worst(alt, want).items():
        big = max(big, v)
        within(f"map_tradeoff (plain tiles) vs numpy.linalg, {k}, {tag}", v, BAR)
    print(f"\n[measured] {tag}: largest error of both tile forms against numpy.linalg {big:.3e}")
    A.free()


@pytest.mark.parametrize("shape,azim", [((17, 11), False), ((11, 7), True), ((13, 3), True)], ids=["iso-135", "azim-135", "azim-33"])
def test_dof_is_map_posteriors_trace(ctx, shape, azim):
    """the point scale 1, damping factor 1 factors dazim_map_posterior's own matrices: sum_b dof per period against its trace (fp32 per
    block and period), and per block, within the bar"""
    prob, _, _, _ = case(shape, azim, mref.REGS[0], 3)
    A = matrix(ctx, prob)
    post = ctx.map_posterior(A, prob["m_data"], prob["nx"], prob["ny"], 3, azim, prob["damp"])
    one = call(ctx, A, prob, np.ones((1, 3 if azim else 1), np.float32), np.array([prob["damp"]], np.float32))
    A.free()
    tr = np.asarray(post["trace"], np.float64)              # [nblk][kmax]
    dof = one["dof"][0].T                                    # [nblk][kmax]
    within(f"map_tradeoff sum of dof per period vs map_posterior's trace, {shape}", np.abs(dof.sum(axis=0) - tr.sum(axis=0)).max() / max(1.0, tr.sum(axis=0).max()), BAR)
    within(f"map_tradeoff dof per block and period vs map_posterior's trace, {shape}", np.abs(dof - tr).max() / max(1.0, tr.max()), BAR)


def test_a_period_that_cannot_be_factored_is_nan_alone(ctx):
    """period 1 has no regularisation rows: at damp 0 the cell no ray crosses leaves its A singular -- NaN and n_failed 1 at that
    (point, period) only, and its neighbours in the sweep have the bits they have without it"""
    prob = ref.problem(9, 5, 3, True, (0.8, 0.0), no_reg_period=1)
    scale, damp = np.ones((3, 3), np.float32), np.array([0.5, 0.0, 0.3], np.float32)
    want = ref.linalg(prob, scale, damp)
    hole = np.zeros((3, 3), np.int32)
    hole[1, 1] = 1
    assert np.array_equal(want["n_failed"], hole)
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, scale, damp)
    clean = call(ctx, A, prob, scale[[0, 2]], damp[[0, 2]])
    A.free()
    assert np.array_equal(got["n_failed"], hole)
    x = got["x"].reshape(3, 3, 3, -1)                        # [K][nblk][kmax][ncell]
    assert np.isnan(x[1, :, 1]).all() and np.isfinite(np.delete(x, 1, axis=2)).all() and np.isfinite(x[[0, 2]]).all()
    for k in ref.PER_PERIOD:
        assert np.isnan(got[k][1, 1]).all() and np.isfinite(np.delete(got[k], 1, axis=1)).all() and np.isfinite(got[k][[0, 2]]).all(), k
    for k, v in ref.worst(got, want).items():
        within(f"map_tradeoff beside a failed period vs numpy.linalg, {k}", v, BAR)
    same_bits(clean, got, ib=[0, 2])
    for k in ref.TOTALS:
        assert np.isnan(got["total"][k][1]) and np.isfinite(got["total"][k][[0, 2]]).all(), k


def test_a_prior_that_is_not_positive_definite_has_no_evidence(ctx):
    """one cell, three blocks: smooth 0 on the a1 block and damp 0 leave P with a zero pivot while A is definite -- logdet_p and logev
    NaN in every period of that point, everything else finite and the reference's, n_failed 0"""
    prob = ref.problem(3, 3, 3, True, (0.7, 0.3))
    scale, damp = np.array([[1, 1, 1], [1, 0, 1], [2, 2, 2]], np.float32), np.array([0.3, 0.0, 0.3], np.float32)
    want = ref.linalg(prob, scale, damp)
    assert not want["n_failed"].any() and np.isnan(want["logev"][1]).all() and np.isfinite(want["chi2"]).all()
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, scale, damp)
    A.free()
    assert not got["n_failed"].any()
    assert np.isnan(got["logdet_p"][1]).all() and np.isnan(got["logev"][1]).all() and np.isfinite(got["logev"][[0, 2]]).all()
    for k in ("chi2", "reg2", "xnorm2", "logdet_a", "dof", "gcv", "x"):
        assert np.isfinite(got[k]).all(), k
    for k, v in ref.worst(got, want).items():
        within(f"map_tradeoff with a semi-definite prior vs numpy.linalg, {k}", v, BAR)


def test_a_period_without_data_follows_the_formulas(ctx):
    """the data rows of period 1 lose their triplets: m_p = 0, x = 0 exactly, chi2 = 0, dof = 0; the other periods have the bits they
    have with them"""
    full = ref.problem(9, 5, 3, True, mref.REGS[0])
    prob = ref.without_data(full, 1)
    scale, damp = ref.sweep(prob)
    scale, damp = scale[:5], damp[:5]
    want = ref.linalg(prob, scale, damp)
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, scale, damp)
    A.free()
    A = matrix(ctx, full)
    whole = call(ctx, A, full, scale, damp)
    A.free()
    assert got["mdata_p"][1] == 0 and not got["n_failed"].any() and ctx.stat("map_trade.grams") == 3
    x = got["x"].reshape(5, 3, 3, -1)
    assert (x[:, :, 1] == 0).all() and (got["chi2"][:, 1] == 0).all() and (got["dof"][:, 1] == 0).all() and (got["xnorm2"][:, 1] == 0).all()
    for k, v in ref.worst(got, want).items():
        within(f"map_tradeoff with a period without data vs numpy.linalg, {k}", v, BAR)
    for k in ref.PER_PERIOD:
        assert np.array_equal(bits(got[k][:, [0, 2]]), bits(whole[k][:, [0, 2]])), k


SENTINEL = -7.5
F64 = ("chi2", "reg2", "xnorm2", "logdet_a", "logdet_p", "dof", "gcv", "logev")


def raw_call(ctx, A, prob, K=2, m_data=None, nx=None, ny=None, kmax=None, azim=None, missing=(), b=True, scale=None, damp=None, want_dof=1,
             want_evidence=1):
    nblk = 3 if prob["azim"] else 1
    n, km = prob["n"], prob["kmax"]
    outs = {k: np.full(2 * km * (nblk if k in ("reg2", "dof") else 1) + 4, SENTINEL) for k in F64}
    outs["x"] = np.full(2 * n + 8, np.float32(SENTINEL))
    outs["n_failed"] = np.full(2 * km + 2, -1, np.int32)
    outs["mdata_p"] = np.full(km + 2, -1, np.int64)
    p = lambda k: None if k in missing else C.c_void_p(outs[k].ctypes.data)
    scale = np.ones((2, nblk), np.float32) if scale is None else np.ascontiguousarray(scale, np.float32)
    damp = np.array([0.3, 0.6], np.float32) if damp is None else np.ascontiguousarray(damp, np.float32)
    rc = ctx.lib.dazim_map_tradeoff(ctx._h, A._h, C.c_int64(prob["m_data"] if m_data is None else m_data),
                                    C.c_void_p(prob["b"].ctypes.data) if b else None, prob["nx"] if nx is None else nx,
                                    prob["ny"] if ny is None else ny, km if kmax is None else kmax,
                                    int(prob["azim"] if azim is None else azim), K, None if "scale" in missing else C.c_void_p(scale.ctypes.data),
                                    None if "damp" in missing else C.c_void_p(damp.ctypes.data), want_dof, want_evidence, p("mdata_p"), p("chi2"),
                                    p("reg2"), p("xnorm2"), p("logdet_a"), p("logdet_p"), p("dof"), p("gcv"), p("logev"), p("x"), p("n_failed"))
    return rc, outs


def untouched(outs):
    return all((o == o.dtype.type(-1 if k in ("n_failed", "mdata_p") else SENTINEL)).all() for k, o in outs.items())


REFUSALS = {"m_data<0": dict(m_data=-1), "m_data>m": dict(m_data=10 ** 6), "n": dict(nx=8), "nx<3": dict(nx=2), "ny<3": dict(ny=2),
            "kmax<1": dict(kmax=0), "kmax": dict(kmax=2), "iso on an azim matrix": dict(azim=0), "K<1": dict(K=0), "no b": dict(b=False),
            "no scale": dict(missing=("scale",)), "no damp": dict(missing=("damp",)), "no chi2": dict(missing=("chi2",)),
            "no reg2": dict(missing=("reg2",)), "no xnorm2": dict(missing=("xnorm2",)), "no logdet_a": dict(missing=("logdet_a",)),
            "scale<0": dict(scale=[[1, 1, 1], [1, -0.5, 1]]), "scale nan": dict(scale=[[1, float("nan"), 1], [1, 1, 1]]),
            "scale inf": dict(scale=[[1, 1, 1], [1, 1, float("inf")]]), "damp<0": dict(damp=[0.3, -0.1]), "damp nan": dict(damp=[float("nan"), 0.1]),
            "damp inf": dict(damp=[0.3, float("inf")]), "gcv without want_dof": dict(want_dof=0, missing=("dof",)),
            "dof without want_dof": dict(want_dof=0, missing=("gcv",)), "logev without want_evidence": dict(want_evidence=0, missing=("logdet_p",)),
            "logdet_p without want_evidence": dict(want_evidence=0, missing=("logev",))}


@pytest.mark.parametrize("bad", sorted(REFUSALS))
def test_refusals(ctx, bad):
    """each refused call returns DAZIM_E_BAD_ARG through the raw entry and writes nothing; a good call follows and writes its K points"""
    prob, _, _, _ = case((9, 5), True, (0.7, 0.3), 3)
    n = prob["n"]
    A = matrix(ctx, prob)
    rc, outs = raw_call(ctx, A, prob, **REFUSALS[bad])
    assert rc == dz.DAZIM_E_BAD_ARG and untouched(outs), bad
    rc, outs = raw_call(ctx, A, prob)
    assert rc == 0 and list(outs["n_failed"]) == [0] * 6 + [-1, -1] and (outs["mdata_p"][:3] > 0).all() and (outs["mdata_p"][3:] == -1).all()
    for k in F64:
        cnt = 18 if k in ("reg2", "dof") else 6
        assert np.isfinite(outs[k][:cnt]).all() and (outs[k][:cnt] != SENTINEL).all() and (outs[k][cnt:] == SENTINEL).all(), k
    assert (outs["x"][:2 * n] != np.float32(SENTINEL)).all() and (outs["x"][2 * n:] == np.float32(SENTINEL)).all()
    rc, outs = raw_call(ctx, A, prob, want_dof=0, want_evidence=0, missing=("dof", "gcv", "logdet_p", "logev", "x", "n_failed", "mdata_p"))
    assert rc == 0 and all((outs[k] == SENTINEL).all() for k in ("dof", "gcv", "logdet_p", "logev")) and (outs["chi2"][:6] > 0).all()
    A.free()


def broken(ctx, prob, row1, col1, word):
    bad = dict(prob, irow=np.append(prob["irow"], row1).astype(np.int32), icol=np.append(prob["icol"], col1).astype(np.int32),
               rw=np.append(prob["rw"], np.float32(0.25)))
    A = matrix(ctx, bad)
    rc, outs = raw_call(ctx, A, bad)
    assert rc == dz.DAZIM_E_BAD_ARG and untouched(outs)
    assert word in ctx.lib.dazim_last_error(ctx._h).decode()
    A.free()


def test_a_regularisation_row_in_two_blocks_is_refused(ctx):
    """found on the device: the first regularisation row (block c, period 0, cell 0) gets an entry in block a2 of the same period"""
    prob, _, _, _ = case((9, 5), True, (0.7, 0.3), 3)
    kn = prob["n"] // 3
    broken(ctx, prob, prob["m_data"] + 1, 2 * kn + 1, "two blocks")


def test_a_row_in_two_periods_is_refused(ctx):
    prob, _, _, _ = case((9, 5), True, (0.7, 0.3), 3)
    ncell = 7 * 3
    at = np.flatnonzero(prob["irow"] == 1)
    per = ((prob["icol"][at[0]] - 1) % (3 * ncell)) // ncell
    broken(ctx, prob, 1, prob["n"] - (ncell if per == 2 else 0), "two periods")   # (the last cell of a map is crossed by no row)


def test_a_row_whose_columns_do_not_ascend_is_refused(ctx):
    prob, _, _, _ = case((9, 5), True, (0.7, 0.3), 3)
    at = np.flatnonzero(prob["irow"] == 1)[0]
    broken(ctx, prob, 1, prob["icol"][at], "ascend")
