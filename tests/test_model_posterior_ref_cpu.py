"""CPU: the two NumPy statements of dazim_model_posterior (tests/model_posterior_ref.py) against each other, the bounds any definite
regulariser implies, the one-knot case against the statements of dazim_map_posterior (tests/map_posterior_ref.py), the Tikhonov rule,
and the condition of every problem the GPU tests run on (cond(A_n) <= 1e4: the fp64 factorisation error stays far below the fp32
rounding of the outputs, so the GPU bar measures the kernels and not the problems)."""
import functools

import numpy as np
import pytest

from tests import map_posterior_ref as mref
from tests import model_posterior_ref as ref

CASES = [(s, False) for s in ref.SHAPES_ISO] + [(s, True) for s in ref.SHAPES_JOINT]
CASE_IDS = [f"{'joint' if jt else 'iso'}-{nx}x{ny}x{nz}" for (nx, ny, nz), jt in CASES]


def seed_of(shape, joint):
    return shape[0] * 10000 + shape[1] * 100 + shape[2] + 7 * joint


@functools.lru_cache(maxsize=None)
def make(shape, joint, reg):
    return ref.problem(shape[0], shape[1], shape[2], joint, reg[0], reg[1], seed=seed_of(shape, joint))


@pytest.mark.parametrize("reg", ref.REGS, ids=ref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_two_forms_agree_and_bounds_hold(case, reg):
    shape, joint = case
    prob = make(shape, joint, reg)
    n = ref.dims(prob)[5]
    assert prob["n"] == n
    sel = np.arange(n)
    a, b = ref.linalg(prob, sel), ref.route(prob, sel)
    assert a["n_failed"] == b["n_failed"] == 0
    for k, v in ref.worst(b, a).items():
        assert v <= 1e-10, (k, v)
    assert (a["std_noise"] <= a["std_post"] * (1 + 1e-12)).all()
    assert (a["trace"] >= -1e-12).all() and a["trace"].sum() < prob["m_data"]
    assert (a["width_h"] >= 0).all() and (a["width_z"] >= 0).all()
    if joint:
        assert (a["leak"] >= 0).all() and (a["leak"] <= 1).all()
    else:
        assert a["leak"] is None
    if reg[0] == 0.0:
        assert (a["rdiag"] >= -1e-12).all() and (a["rdiag"] < 1).all()
    if prob["dead"] is not None and reg[0] == 0.0:           # damping alone: a cell without rays resolves nothing, prior std 1 / damp
        j, i = divmod(prob["dead"], shape[0] - 2)
        assert np.allclose(a["rdiag"][:, :, j, i], 0.0, atol=1e-14) and np.allclose(a["std_post"][:, :, j, i], 1 / prob["damp"])


@pytest.mark.parametrize("reg", ref.REGS, ids=ref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_condition_of_the_gpu_problems(case, reg):
    """a condition, not a measurement: the GPU bar of 1e-6 is the project's for this arithmetic at cond <= 1e4"""
    shape, joint = case
    prob = make(shape, joint, reg)
    assert np.linalg.cond(ref.normal_matrix(prob, *ref.parts(prob))) <= ref.COND_MAX


@pytest.mark.parametrize("case", [c for c in CASES if c[0][2] == 2], ids=[i for c, i in zip(CASES, CASE_IDS) if c[0][2] == 2])
def test_one_knot_is_the_map_statement(case):
    """nz = 2: one knot, the 3-D layout is the map layout of one period, and the outputs are map_posterior_ref's for kmax = 1"""
    shape, joint = case
    prob = make(shape, joint, ref.REGS[0])
    mprob = dict(nx=prob["nx"], ny=prob["ny"], kmax=1, azim=prob["joint"], damp=prob["damp"], m=prob["m"], m_data=prob["m_data"],
                 n=prob["n"], irow=prob["irow"], icol=prob["icol"], rw=prob["rw"])
    sel = np.arange(prob["n"])
    for fn, mfn in ((ref.linalg, mref.linalg), (ref.route, mref.route)):
        a, b = fn(prob, sel), mfn(mprob, sel)
        for k, mk in (("std_post", "std_post"), ("std_noise", "std_noise"), ("rdiag", "rdiag"), ("rsum", "rsum"), ("width_h", "width"),
                      ("leak", "leak"), ("trace", "trace")):
            if a[k] is None:
                assert b[mk] is None
                continue
            assert np.abs(a[k] - b[mk]).max() <= 1e-12 * max(1.0, np.abs(b[mk]).max()), k
        assert np.abs(a["rows"] - b["rows"][0]).max() <= 1e-12
        assert not a["width_z"].any()


@pytest.mark.parametrize("joint", [False, True], ids=["iso", "joint"])
def test_rows_are_the_solves_resolution(joint):
    """noise-free data d = G z of a true model z, solved by the dense normal equations with the regulariser: x = Rm z"""
    prob = make((8, 7, 6), joint, (0.7, 0.3))
    n = prob["n"]
    want = ref.linalg(prob, np.arange(n))
    D, L = ref.parts(prob)
    z = np.random.default_rng(5).normal(size=n)
    x = np.linalg.solve(ref.normal_matrix(prob, D, L), D @ z)
    assert np.abs(x - want["rows"] @ z).max() <= 1e-10 * max(1.0, np.abs(x).max())


def test_singular_matrix_is_nan_in_both_forms():
    prob = ref.problem(9, 5, 3, True, 0.0, 0.0, seed=1)
    for fn in (ref.linalg, ref.route):
        out = fn(prob, np.array([0, 3]))
        assert out["n_failed"] == 1
        for k in ref.OUTPUTS:
            assert np.isnan(out[k]).all(), k


def test_tikhonov_rule():
    nx, ny, nz = 6, 5, 4                                     # 4 x 3 x 3 cells, two inner ones
    r, c, v = ref.tikhonov3d(nx, ny, nz, [0.5, 2.0])
    ncell, maxvp = 12, 36
    A = np.zeros((2 * maxvp, 2 * maxvp))
    A[r, c] = v
    assert A[0, 0] == 1.0 and A[maxvp + 3, maxvp + 3] == 4.0
    inner = 1 * ncell + 1 * 4 + 1                            # knot 1, j 1, i 1
    assert A[inner, inner] == 3.0
    assert sorted(np.flatnonzero(A[inner])) == [inner - ncell, inner - 4, inner - 1, inner, inner + 1, inner + 4, inner + ncell]
    assert A[inner].sum() == 0.0 and not A[:maxvp, maxvp:].any() and not A[maxvp:, :maxvp].any()
    assert (np.count_nonzero(A, axis=1) == 7).sum() == 2 * 2 and (np.diff(r) >= 0).all()
