"""-m gpu: dazim_model_posterior: posterior std, resolution matrix and what is derived from it per block, knot
and inner cell of the direct 3-D inversion, from the matrix LSMR is given.

Against numpy.linalg (tests/model_posterior_ref.py) at the sizes the panel width 32 and the 64-tile set (n = 1, 31, 32, 33, 65, 135,
150 in iso-mode; 3, 30, 33, 63, 66, 135, 450 in joint mode), three regularisers, both tile forms; the arguments that may be left out,
host against device arrays, a second call, dazim_map_posterior on a one-knot problem, a matrix that cannot be factored, the refused
calls, and the rows of a small synthetic survey."""
import ctypes as C
import functools

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import map_posterior_ref as mref
from tests import model_posterior_ref as ref
from tests.bars import within

pytestmark = pytest.mark.gpu

CASES = [(s, False) for s in ref.SHAPES_ISO] + [(s, True) for s in ref.SHAPES_JOINT]
CASE_IDS = [f"{'joint' if jt else 'iso'}-{nx}x{ny}x{nz}" for (nx, ny, nz), jt in CASES]
BAR = 1e-6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def some_sel(n):
    return np.unique(np.array([0, n // 2, n - 1, n // 3], np.int32))


@functools.lru_cache(maxsize=None)
def case(shape, joint, reg):
    """the problem tests/test_model_posterior_ref_cpu.py bounds the condition of (same generator, same seed), and its reference"""
    prob = ref.problem(shape[0], shape[1], shape[2], joint, reg[0], reg[1], seed=shape[0] * 10000 + shape[1] * 100 + shape[2] + 7 * joint)
    for k in ("irow", "icol", "rw", "depz"):
        prob[k].setflags(write=False)
    return prob, ref.linalg(prob, some_sel(prob["n"]))


def matrix(ctx, prob):
    return ctx.csr_from_coo(prob["m"], prob["n"], prob["irow"], prob["icol"], prob["rw"])


def call(ctx, A, prob, sel=None, width=True, depz=True):
    return ctx.model_posterior(A, prob["m_data"], prob["nx"], prob["ny"], prob["nz"], prob["joint"], prob["damp"],
                               depz=prob["depz"] if depz else None, sel=sel, width=width)


def same_bits(a, b, keys):
    for k in keys:
        if a[k] is None or b[k] is None:
            continue
        x = a[k].cpu().numpy() if dz._is_torch(a[k]) else a[k]
        y = b[k].cpu().numpy() if dz._is_torch(b[k]) else b[k]
        assert np.array_equal(bits(x), bits(y)), k


@pytest.mark.parametrize("reg", ref.REGS, ids=ref.REG_IDS)
@pytest.mark.parametrize("shape,joint", CASES, ids=CASE_IDS)
def test_equals_numpy_linalg(ctx, shape, joint, reg):
    """every output within 1e-6 * max(1, max |reference|) of numpy.linalg, with either tile form (the largest value is printed); a
    second call, a torch device sel, and a call without sel, rows and the widths give the same bits.
    Measured on an MI355X, largest over the 42 cases and both tile forms: 5.6e-8 (bar 1e-6)."""
    import torch
    prob, want = case(shape, joint, reg)
    n = prob["n"]
    sel = some_sel(n)
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, sel)
    assert got["n_failed"] == 0 and ctx.stat("model_post.n") == n
    tag = f"{'joint' if joint else 'iso'} n {n}"
    big = 0.0
    for k, v in ref.worst(got, want).items():
        big = max(big, v)
        within(f"model_posterior vs numpy.linalg, {k}, {tag}", v, BAR)
    same_bits(call(ctx, A, prob, sel), got, ref.OUTPUTS)
    dev = call(ctx, A, prob, torch.from_numpy(sel).cuda())
    assert dz._is_torch(dev["std_post"]) and dev["n_failed"] == 0
    same_bits(dev, got, ref.OUTPUTS)
    lean = call(ctx, A, prob, None, width=False)
    assert lean["rows"] is None and lean["width_h"] is None and lean["width_z"] is None
    same_bits(lean, got, ("std_post", "std_noise", "rdiag", "rsum", "leak", "trace"))
    nodepth = call(ctx, A, prob, sel, depz=False)
    assert nodepth["width_z"] is None
    same_bits(nodepth, got, ("std_post", "std_noise", "rdiag", "rsum", "width_h", "leak", "trace", "rows"))
    ctx.set_option("map_post.mfma", 0)                     # the plain tile form
    try:
        alt = call(ctx, A, prob, sel)
    finally:
        ctx.set_option("map_post.mfma", 1)
    for k, v in ref.worst(alt, want).items():
        big = max(big, v)
        within(f"model_posterior (plain tiles) vs numpy.linalg, {k}, {tag}", v, BAR)
    print(f"\n[measured] {tag}: largest error of both tile forms against numpy.linalg {big:.3e}")
    A.free()


@pytest.mark.parametrize("azim", [False, True], ids=["iso", "joint"])
def test_one_knot_is_the_map_call(ctx, azim):
    """one of map_posterior_ref's own kmax = 1 problems (n_g 33 and 99; its regularisation rows are the 2-D five-point ones, not
    dazim_csr_append_tikhonov's): dazim_model_posterior with nz = 2 and dazim_map_posterior on the same matrix.  The normal matrix and
    the dense part are the same kernels on the same numbers, and the two row passes subtract the same products t_l l_c in the same
    order and sum along the row in the same stride (MpRowSum, map_post_internal.h): every output equal bit for bit.  Measured on an
    MI355X, on the commit before the row pass was stated once and on it: all values equal in every output, 33 + 99 per unknown, 132 +
    396 of the rows, 1 + 3 of the trace (profiles/posterior_rows_refactor.md)."""
    mprob = mref.problem(13, 5, 1, azim, 0.7, 0.3, seed=11)
    n = mprob["n"]
    sel = some_sel(n)
    A = ctx.csr_from_coo(mprob["m"], n, mprob["irow"], mprob["icol"], mprob["rw"])
    a = ctx.map_posterior(A, mprob["m_data"], 13, 5, 1, azim, mprob["damp"], sel=sel)
    b = ctx.model_posterior(A, mprob["m_data"], 13, 5, 2, azim, mprob["damp"], depz=np.zeros(1, np.float32), sel=sel)
    A.free()
    assert a["n_failed"] == b["n_failed"] == 0
    assert not b["width_z"].any()
    pairs = [("std_post", "std_post"), ("std_noise", "std_noise"), ("rdiag", "rdiag"), ("rsum", "rsum"), ("width_h", "width"), ("trace", "trace"),
             ("rows", "rows")] + ([("leak", "leak")] if azim else [])
    for k, mk in pairs:
        x, y = bits(b[k]).reshape(-1), bits(a[mk]).reshape(-1)
        print(f"\n[measured] n {n}: {k} against dazim_map_posterior, {x.size} values: {int((x == y).sum())} equal")
        assert np.array_equal(x, y), k


def test_a_matrix_that_cannot_be_factored_is_nan_and_counted(ctx):
    """smoothing 0, damping 0 and a cell without rays: every output NaN and n_failed 1"""
    prob = ref.problem(9, 5, 3, True, 0.0, 0.0, seed=1)
    sel = some_sel(prob["n"])
    assert ref.linalg(prob, sel)["n_failed"] == 1
    A = matrix(ctx, prob)
    got = call(ctx, A, prob, sel)
    A.free()
    assert got["n_failed"] == 1
    for k in ref.OUTPUTS:
        assert np.isnan(got[k]).all(), k


SENTINEL = np.float32(-7.5)
PER = ("std_post", "std_noise", "rdiag", "rsum", "width_h", "width_z", "leak")


def raw_call(ctx, A, prob, m_data=None, nx=None, ny=None, nz=None, joint=None, missing=None, leak=None, sel=None, rows=False, damp=None,
             depz=True, width_z=True):
    nblk = 3 if prob["joint"] else 1
    n = prob["n"]
    outs = {k: np.full(n + 8, SENTINEL) for k in PER}
    outs["rows"] = np.full(4 * n, SENTINEL)
    outs["trace"] = np.full(nblk * (prob["nz"] - 1), SENTINEL)
    p = lambda k: None if k == missing else C.c_void_p(outs[k].ctypes.data)
    use_leak = prob["joint"] if leak is None else leak
    sel = None if sel is None else np.ascontiguousarray(sel, np.int32)
    nf = C.c_int(-1)
    rc = ctx.lib.dazim_model_posterior(ctx._h, A._h, C.c_int64(prob["m_data"] if m_data is None else m_data), prob["nx"] if nx is None else nx,
                                       prob["ny"] if ny is None else ny, prob["nz"] if nz is None else nz,
                                       int(prob["joint"] if joint is None else joint), C.c_float(prob["damp"] if damp is None else damp),
                                       C.c_void_p(prob["depz"].ctypes.data) if depz else None, p("std_post"), p("std_noise"), p("rdiag"),
                                       p("rsum"), p("width_h"), p("width_z") if width_z else None, p("leak") if use_leak else None,
                                       0 if sel is None else len(sel), None if sel is None else C.c_void_p(sel.ctypes.data),
                                       p("rows") if rows else None, p("trace"), C.byref(nf))
    return rc, nf.value, outs


REFUSALS = {"m_data<0": dict(m_data=-1), "m_data>m": dict(m_data=10 ** 6), "n": dict(nx=8), "nx<3": dict(nx=2), "ny<3": dict(ny=2),
            "nz<2": dict(nz=1), "no std_post": dict(missing="std_post"), "no std_noise": dict(missing="std_noise"),
            "no rdiag": dict(missing="rdiag"), "no rsum": dict(missing="rsum"), "width_z without depz": dict(depz=False),
            "depz without width_z": dict(width_z=False), "sel<0": dict(sel=[0, -1]), "sel>=n": dict(sel=[1, 10 ** 4]),
            "rows without sel": dict(rows=True), "damp<0": dict(damp=-0.1), "damp nan": dict(damp=float("nan")),
            "damp inf": dict(damp=float("inf"))}


@pytest.mark.parametrize("bad", sorted(REFUSALS))
def test_refusals(ctx, bad):
    """each refused call returns DAZIM_E_BAD_ARG through the raw entry and writes nothing; a good call follows"""
    prob, _ = case((7, 5, 4), True, (0.7, 0.3))
    n = prob["n"]
    A = matrix(ctx, prob)
    rc, nf, outs = raw_call(ctx, A, prob, **REFUSALS[bad])
    assert rc == dz.DAZIM_E_BAD_ARG and nf == -1 and all((o == SENTINEL).all() for o in outs.values()), bad
    rc, nf, outs = raw_call(ctx, A, prob, sel=[2, 5], rows=True)
    assert rc == 0 and nf == 0 and (outs["std_post"][:n] > 0).all() and (outs["std_post"][n:] == SENTINEL).all()
    assert (outs["rows"][:2 * n] != SENTINEL).all() and (outs["rows"][2 * n:] == SENTINEL).all()
    A.free()


def test_leak_without_joint_is_refused(ctx):
    prob, _ = case((11, 7, 4), False, (0.7, 0.3))
    A = matrix(ctx, prob)
    rc, nf, outs = raw_call(ctx, A, prob, leak=True)
    assert rc == dz.DAZIM_E_BAD_ARG and nf == -1 and all((o == SENTINEL).all() for o in outs.values())
    assert "leak" in ctx.lib.dazim_last_error(ctx._h).decode()
    rc, nf, outs = raw_call(ctx, A, prob)
    assert rc == 0 and nf == 0 and (outs["leak"] == SENTINEL).all()
    A.free()


def test_a_workspace_the_card_cannot_hold_is_refused(ctx):
    """n = 500 x 300 cells at one knot: two n x n fp64 matrices are 335 GiB, more than an MI355X has; refused before anything is
    allocated or launched, with the GiB needed in the message"""
    nx, ny, n = 502, 302, 150000
    A = ctx.csr_from_coo(3, n, np.array([1, 2, 3], np.int32), np.array([1, 7, n], np.int32), np.ones(3, np.float32))
    with pytest.raises(dz.DazimError) as e:
        ctx.model_posterior(A, 3, nx, ny, 2, False, 0.5)
    assert e.value.code == dz.DAZIM_E_BAD_ARG and "GiB" in str(e.value) and "335." in str(e.value)
    A.free()


@pytest.mark.parametrize("where", ["data row", "regularisation row"])
def test_a_row_whose_columns_do_not_ascend_is_refused(ctx, where):
    """found on the device: a repeated triplet leaves a column twice in its row"""
    prob, _ = case((7, 5, 4), True, (0.7, 0.3))
    row = 1 if where == "data row" else prob["m"]
    at = np.flatnonzero(prob["irow"] == row)[0]
    bad = dict(prob, irow=np.append(prob["irow"], row).astype(np.int32), icol=np.append(prob["icol"], prob["icol"][at]).astype(np.int32),
               rw=np.append(prob["rw"], np.float32(0.25)))
    A = matrix(ctx, bad)
    rc, nf, outs = raw_call(ctx, A, bad)
    assert rc == dz.DAZIM_E_BAD_ARG and nf == -1 and all((o == SENTINEL).all() for o in outs.values())
    assert "ascend" in ctx.lib.dazim_last_error(ctx._h).decode()
    A.free()


@pytest.mark.parametrize("joint", [False, True], ids=["iso", "joint"])
def test_rows_of_a_synthetic_survey(ctx, joint):
    """real rows: the grid and stations of tests/test_column_lsq_gpu.py's small survey (11 x 9 vertices, 4 knots, 2 periods),
    rays_build_G / its joint mode, weighted and regularised as the program does (dazim_weight_data, dazim_csr_append_tikhonov, damping
    0.01); the triplets taken back through to_coo for the reference.  Measured on an MI355X (480 rays): iso n 189, cond(A_n) 3.3e1,
    largest over the outputs 4.5e-8; joint n 567, cond(A_n) 1.1e2, largest 4.5e-8; median std_post of Vs per knot 0.25, 0.11, 0.24 km/s."""
    from tests.test_column_lsq_gpu import DV, GOXD, GOZD, layered_model, survey
    nx, ny, kmax, damp = 11, 9, 2, 0.01
    depz = np.array([0.0, 6.0, 16.0, 32.0], np.float32)
    nz = len(depz)
    tRc = np.array([8.0, 20.0])
    vel = layered_model(nx, ny, depz, seed=5)
    pv, sen, nf = ctx.depthkernel(vel, depz, tRc, 2.0)
    assert nf == 0
    lsen = ctx.ti_kernels(vel, depz, tRc, 2.0, pv) if joint else None
    scx, scz, per, ray_f, rx, rz = survey(nx, ny, kmax, 10, None, seed=21)
    fields = ctx.fmm_batch(nx, ny, GOXD, GOZD, DV, DV, pv, scx, scz, per)
    G, tp, _ = ctx.rays_build_G(nx, ny, GOXD, GOZD, DV, DV, vel, fields, scx, scz, per, ray_f, rx, rz, sen, lsen=lsen)
    m_data = G.m
    tp = tp.copy()
    tobs = (tp + np.random.default_rng(4).normal(0.0, 0.3, len(tp))).astype(np.float32)
    ctx.weight_data(G, tobs, tp)
    G.append_tikhonov(nx, ny, nz, np.array([2.0, 4.0, 4.0][:3 if joint else 1], np.float32))
    irow, icol, rw = G.to_coo()
    prob = dict(nx=nx, ny=ny, nz=nz, joint=joint, damp=float(np.float32(damp)), m=G.m, m_data=m_data, n=G.n, irow=irow, icol=icol, rw=rw,
                depz=depz[:nz - 1].copy())
    sel = some_sel(prob["n"])
    got = call(ctx, G, prob, sel)
    G.free()
    want = ref.linalg(prob, sel)
    cond = np.linalg.cond(ref.normal_matrix(prob, *ref.parts(prob)))
    worst = ref.worst(got, want)
    print(f"\n[measured] synthetic survey, {'joint' if joint else 'iso'}: {m_data} rays, n {prob['n']}, cond(A_n) {cond:.2e}, largest error "
          f"{max(worst.values()):.3e}, median std_post(Vs) per knot {np.median(got['std_post'][0].reshape(nz - 1, -1), axis=1)}, median "
          f"width_h {np.median(got['width_h'][0]):.2f} cells, width_z {np.median(got['width_z'][0]):.2f} km")
    assert got["n_failed"] == want["n_failed"] == 0
    for k, v in worst.items():
        within(f"model_posterior vs numpy.linalg on a synthetic survey, {k}", v, BAR)
