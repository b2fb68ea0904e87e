"""-m gpu: dazim_model_tradeoff: the linearised step of the direct 3-D inversion solved exactly at every point of
a sweep over regularisation strengths, with chi2, the regularisation norms, log-determinants, degrees of freedom, GCV and the evidence.

Against numpy.linalg (tests/model_tradeoff_ref.py) on model_posterior_ref's problems (n = 1, 31, 32, 33, 65, 135, 150 in iso-mode; 3,
30, 33, 63, 66, 135, 450 in joint mode: both sides of the panel width 32 and of the 64-tile), three regularisers, both tile forms; bit
equality of a second call, a device right-hand side, every point alone, the sweep reversed and the calls with dof or evidence off;
dazim_model_posterior's trace; a point that cannot be factored; a prior that is not positive definite; the refused calls; the picks."""
import ctypes as C
import functools

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import model_posterior_ref as mref
from tests import model_tradeoff_ref as ref
from tests.bars import within

pytestmark = pytest.mark.gpu

CASES = [(s, False) for s in mref.SHAPES_ISO] + [(s, True) for s in mref.SHAPES_JOINT]
CASE_IDS = [f"{'joint' if jt else 'iso'}-{nx}x{ny}x{nz}" for (nx, ny, nz), jt in CASES]
BAR = 1e-6   # the bar of tests/test_model_posterior_gpu.py for these dense kernels


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def case(shape, joint, reg):
    """the problem and sweep tests/test_model_tradeoff_ref_cpu.py bounds the condition of, and its reference"""
    prob = ref.problem(shape, joint, reg)
    scale, damp = ref.sweep(prob)
    for a in (prob["irow"], prob["icol"], prob["rw"], prob["b"], scale, damp):
        a.setflags(write=False)
    return prob, scale, damp, ref.linalg(prob, scale, damp)


def matrix(ctx, prob):
    return ctx.csr_from_coo(prob["m"], prob["n"], prob["irow"], prob["icol"], prob["rw"])


def call(ctx, A, prob, scale, damp, b=None, **kw):
    kw.setdefault("x", True)
    return ctx.model_tradeoff(A, prob["m_data"], prob["b"] if b is None else b, prob["nx"], prob["ny"], prob["nz"], prob["joint"], scale, damp, **kw)


def same_bits(a, b, keys=ref.OUTPUTS, ia=slice(None), ib=slice(None)):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(bits(a[k][ia]), bits(b[k][ib])), k
    assert np.array_equal(a["n_failed"][ia], b["n_failed"][ib])


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("shape,joint", CASES, ids=CASE_IDS)
def test_equals_numpy_linalg_and_bits_hold(ctx, shape, joint, reg):
    """every output within 1e-6 * max(1, max |reference|) of numpy.linalg, with either tile form (the largest value is printed); the same
    bits from a second call, a device b, the sweep reversed (which a clobbered D would not survive), every point alone, and from the
    calls without dof or without the evidence in the outputs that remain.
    Measured on an MI355X, largest over the 42 cases and both tile forms: 5.2e-08 (bar 1e-6)."""
    import torch
    prob, scale, damp, want = case(shape, joint, reg)
    n, K = prob["n"], len(damp)
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, scale, damp)
    assert not got["n_failed"].any() and ctx.stat("model_trade.n") == n and ctx.stat("model_trade.points") == K
    tag = f"{'joint' if joint else 'iso'} n {n}"
    big = 0.0
    for k, v in ref.worst(got, want).items():
        big = max(big, v)
        within(f"model_tradeoff vs numpy.linalg, {k}, {tag}", v, BAR)
    assert got["pick"] == ref.pick(got["chi2"], got["reg2"].sum(axis=1), got["gcv"], got["logev"])
    same_bits(call(ctx, A, prob, scale, damp), got)
    same_bits(call(ctx, A, prob, scale, damp, b=torch.from_numpy(prob["b"].copy()).cuda()), got)
    same_bits(call(ctx, A, prob, scale[::-1].copy(), damp[::-1].copy()), got, ib=slice(None, None, -1))
    for k in range(K):
        same_bits(call(ctx, A, prob, scale[k:k + 1], damp[k:k + 1]), got, ib=slice(k, k + 1))
    nodof = call(ctx, A, prob, scale, damp, dof=False)
    assert nodof["dof"] is None and nodof["gcv"] is None
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
        within(f"model_tradeoff (plain tiles) vs numpy.linalg, {k}, {tag}", v, BAR)
    print(f"\n[measured] {tag}: largest error of both tile forms against numpy.linalg {big:.3e}")
    A.free()


@pytest.mark.parametrize("shape,joint", [((11, 7, 4), False), ((7, 5, 4), True), ((8, 7, 6), True)], ids=["iso-135", "joint-135", "joint-450"])
def test_dof_is_model_posteriors_trace(ctx, shape, joint):
    """the point scale 1, damping factor 1 factors dazim_model_posterior's own matrix: sum_b dof against the sum of its trace (fp32
    per block and knot), within the bar"""
    prob, scale, damp, _ = case(shape, joint, mref.REGS[0])
    A = matrix(ctx, prob)
    post = ctx.model_posterior(A, prob["m_data"], prob["nx"], prob["ny"], prob["nz"], joint, prob["damp"])
    one = call(ctx, A, prob, np.ones((1, 3 if joint else 1), np.float32), np.array([prob["damp"]], np.float32))
    A.free()
    tr = float(np.asarray(post["trace"], np.float64).sum())
    within(f"model_tradeoff sum of dof vs model_posterior's trace, n {prob['n']}", abs(one["dof"].sum() - tr) / max(1.0, abs(tr)), BAR)
    per_block = np.asarray(post["trace"], np.float64).sum(axis=1)
    within("model_tradeoff dof per block vs model_posterior's trace per block", np.abs(one["dof"][0] - per_block).max() / max(1.0, per_block.max()), BAR)


def test_a_point_that_cannot_be_factored_is_nan_alone(ctx):
    """no regularisation rows: at damp 0 the cell no ray crosses leaves A_k singular -- NaN and n_failed 1 at that point only, and its
    neighbours in the sweep have the bits they have without it"""
    prob = ref.problem((9, 5, 3), True, (0.0, 0.5))
    scale, damp = np.ones((3, 3), np.float32), np.array([0.5, 0.0, 0.3], np.float32)
    want = ref.linalg(prob, scale, damp)
    assert list(want["n_failed"]) == [0, 1, 0]
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, scale, damp)
    clean = call(ctx, A, prob, scale[[0, 2]], damp[[0, 2]])
    A.free()
    assert list(got["n_failed"]) == [0, 1, 0]
    for k in ref.OUTPUTS:
        assert np.isnan(got[k][1]).all() and np.isfinite(got[k][[0, 2]]).all(), k
    for k, v in ref.worst(got, want).items():
        within(f"model_tradeoff beside a failed point vs numpy.linalg, {k}", v, BAR)
    same_bits(clean, got, ib=[0, 2])
    assert got["pick"] == ref.pick(got["chi2"], got["reg2"].sum(axis=1), got["gcv"], got["logev"]) and got["pick"]["corner"] == -1


def test_a_prior_that_is_not_positive_definite_has_no_evidence(ctx):
    """one cell, three blocks: smooth 0 on the Gc block and damp 0 leave P_k with a zero pivot while A_k is definite -- logdet_p and logev
    NaN, everything else finite and the reference's, n_failed 0"""
    prob = ref.problem((3, 3, 2), True, (0.7, 0.3))
    scale, damp = np.array([[1, 1, 1], [1, 0, 1], [2, 2, 2]], np.float32), np.array([0.3, 0.0, 0.3], np.float32)
    want = ref.linalg(prob, scale, damp)
    assert not want["n_failed"].any() and np.isnan(want["logev"][1]) and np.isfinite(want["chi2"]).all()
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, scale, damp)
    A.free()
    assert not got["n_failed"].any()
    assert np.isnan(got["logdet_p"][1]) and np.isnan(got["logev"][1]) and np.isfinite(got["logev"][[0, 2]]).all()
    for k in ("chi2", "reg2", "xnorm2", "logdet_a", "dof", "gcv", "x"):
        assert np.isfinite(got[k]).all(), k
    for k, v in ref.worst(got, want).items():
        within(f"model_tradeoff with a semi-definite prior vs numpy.linalg, {k}", v, BAR)


SENTINEL = -7.5
F64 = ("chi2", "reg2", "xnorm2", "logdet_a", "logdet_p", "dof", "gcv", "logev")


def raw_call(ctx, A, prob, K=2, m_data=None, nx=None, ny=None, nz=None, joint=None, missing=(), b=True, scale=None, damp=None, want_dof=1,
             want_evidence=1):
    nblk = 3 if prob["joint"] else 1
    n = prob["n"]
    outs = {k: np.full(3 * nblk + 4, SENTINEL) for k in F64}
    outs["x"] = np.full(2 * n + 8, np.float32(SENTINEL))
    outs["n_failed"] = np.full(4, -1, np.int32)
    p = lambda k: None if k in missing else C.c_void_p(outs[k].ctypes.data)
    scale = np.ones((2, nblk), np.float32) if scale is None else np.ascontiguousarray(scale, np.float32)
    damp = np.array([0.3, 0.6], np.float32) if damp is None else np.ascontiguousarray(damp, np.float32)
    rc = ctx.lib.dazim_model_tradeoff(ctx._h, A._h, C.c_int64(prob["m_data"] if m_data is None else m_data),
                                      C.c_void_p(prob["b"].ctypes.data) if b else None, prob["nx"] if nx is None else nx,
                                      prob["ny"] if ny is None else ny, prob["nz"] if nz is None else nz,
                                      int(prob["joint"] if joint is None else joint), K, None if "scale" in missing else C.c_void_p(scale.ctypes.data),
                                      None if "damp" in missing else C.c_void_p(damp.ctypes.data), want_dof, want_evidence, p("chi2"), p("reg2"),
                                      p("xnorm2"), p("logdet_a"), p("logdet_p"), p("dof"), p("gcv"), p("logev"), p("x"), p("n_failed"))
    return rc, outs


REFUSALS = {"m_data<0": dict(m_data=-1), "m_data>m": dict(m_data=10 ** 6), "n": dict(nx=8), "nx<3": dict(nx=2), "ny<3": dict(ny=2),
            "nz<2": dict(nz=1), "iso on a joint matrix": dict(joint=0), "K<1": dict(K=0), "no b": dict(b=False), "no scale": dict(missing=("scale",)),
            "no damp": dict(missing=("damp",)), "no chi2": dict(missing=("chi2",)), "no reg2": dict(missing=("reg2",)),
            "no xnorm2": dict(missing=("xnorm2",)), "no logdet_a": dict(missing=("logdet_a",)),
            "scale<0": dict(scale=[[1, 1, 1], [1, -0.5, 1]]), "scale nan": dict(scale=[[1, float("nan"), 1], [1, 1, 1]]),
            "scale inf": dict(scale=[[1, 1, 1], [1, 1, float("inf")]]), "damp<0": dict(damp=[0.3, -0.1]), "damp nan": dict(damp=[float("nan"), 0.1]),
            "damp inf": dict(damp=[0.3, float("inf")]), "gcv without want_dof": dict(want_dof=0, missing=("dof",)),
            "dof without want_dof": dict(want_dof=0, missing=("gcv",)), "logev without want_evidence": dict(want_evidence=0, missing=("logdet_p",)),
            "logdet_p without want_evidence": dict(want_evidence=0, missing=("logev",))}


@pytest.mark.parametrize("bad", sorted(REFUSALS))
def test_refusals(ctx, bad):
    """each refused call returns DAZIM_E_BAD_ARG through the raw entry and writes nothing; a good call follows and writes its K points"""
    prob, _, _, _ = case((7, 5, 4), True, (0.7, 0.3))
    n = prob["n"]
    A = matrix(ctx, prob)
    rc, outs = raw_call(ctx, A, prob, **REFUSALS[bad])
    assert rc == dz.DAZIM_E_BAD_ARG and all((o == o.dtype.type(-1 if k == "n_failed" else SENTINEL)).all() for k, o in outs.items()), bad
    rc, outs = raw_call(ctx, A, prob)
    assert rc == 0 and list(outs["n_failed"]) == [0, 0, -1, -1]
    for k in F64:
        cnt = 6 if k in ("reg2", "dof") else 2
        assert np.isfinite(outs[k][:cnt]).all() and (outs[k][:cnt] != SENTINEL).all() and (outs[k][cnt:] == SENTINEL).all(), k
    assert (outs["x"][:2 * n] != np.float32(SENTINEL)).all() and (outs["x"][2 * n:] == np.float32(SENTINEL)).all()
    rc, outs = raw_call(ctx, A, prob, want_dof=0, want_evidence=0, missing=("dof", "gcv", "logdet_p", "logev", "x", "n_failed"))
    assert rc == 0 and all((outs[k] == SENTINEL).all() for k in ("dof", "gcv", "logdet_p", "logev")) and (outs["chi2"][:2] > 0).all()
    A.free()


def test_a_regularisation_row_in_two_blocks_is_refused(ctx):
    """found on the device: one regularisation row of the Vs block gets an entry in the Gs block"""
    prob, _, _, _ = case((7, 5, 4), True, (0.7, 0.3))
    bad = dict(prob, irow=np.append(prob["irow"], prob["m_data"] + 1).astype(np.int32), icol=np.append(prob["icol"], prob["n"]).astype(np.int32),
               rw=np.append(prob["rw"], np.float32(0.25)))
    A = matrix(ctx, bad)
    rc, outs = raw_call(ctx, A, bad)
    assert rc == dz.DAZIM_E_BAD_ARG and all((o == o.dtype.type(-1 if k == "n_failed" else SENTINEL)).all() for k, o in outs.items())
    assert "two blocks" in ctx.lib.dazim_last_error(ctx._h).decode()
    A.free()


def test_a_row_whose_columns_do_not_ascend_is_refused(ctx):
    prob, _, _, _ = case((7, 5, 4), True, (0.7, 0.3))
    at = np.flatnonzero(prob["irow"] == 1)[0]
    bad = dict(prob, irow=np.append(prob["irow"], 1).astype(np.int32), icol=np.append(prob["icol"], prob["icol"][at]).astype(np.int32),
               rw=np.append(prob["rw"], np.float32(0.25)))
    A = matrix(ctx, bad)
    rc, outs = raw_call(ctx, A, bad)
    assert rc == dz.DAZIM_E_BAD_ARG and all((o == o.dtype.type(-1 if k == "n_failed" else SENTINEL)).all() for k, o in outs.items())
    assert "ascend" in ctx.lib.dazim_last_error(ctx._h).decode()
    A.free()


def test_a_workspace_the_card_cannot_hold_is_refused(ctx):
    """n = 150000: three n x n fp64 matrices are 503 GiB, more than an MI355X has; refused before anything is allocated or launched,
    with the GiB needed in the message"""
    nx, ny, n = 502, 302, 150000
    A = ctx.csr_from_coo(3, n, np.array([1, 2, 3], np.int32), np.array([1, 7, n], np.int32), np.ones(3, np.float32))
    with pytest.raises(dz.DazimError) as e:
        ctx.model_tradeoff(A, 3, np.ones(3, np.float32), nx, ny, 2, False, [1.0], [0.5])
    assert e.value.code == dz.DAZIM_E_BAD_ARG and "GiB" in str(e.value) and "503." in str(e.value)
    A.free()


def test_pick_is_the_numpy_statement(ctx):
    """the three rules on random sweeps (tests/model_tradeoff_ref.check_pick, which the CPU suite runs too) and on a real one"""
    ref.check_pick(dz.tradeoff_pick)
    prob, scale, damp, _ = case((8, 7, 6), True, mref.REGS[0])
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, scale[:5], damp[:5], x=False)
    A.free()
    want = ref.pick(got["chi2"], got["reg2"].sum(axis=1), got["gcv"], got["logev"])
    assert got["pick"] == want and 0 < want["corner"] < 4 and want["gcv"] >= 0 and want["evidence"] >= 0
