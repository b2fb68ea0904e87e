"""CPU: the two NumPy statements of dazim_map_posterior (tests/map_posterior_ref.py) against each other, the bounds any definite
regulariser implies, the identity that makes Rm the resolution matrix of the regularised solve, and the condition of every problem
the GPU tests run on (cond(A_g) <= 1e6: the fp64 factorisation error stays far below the fp32 rounding of the outputs, so the GPU
bar measures the kernels and not the problems)."""
import numpy as np
import pytest

from tests import map_posterior_ref as ref

CASES = [(s, False) for s in ref.SHAPES_ISO] + [(s, True) for s in ref.SHAPES_JOINT]
CASE_IDS = [f"{'joint' if az else 'iso'}-{nx}x{ny}" for (nx, ny), az in CASES]


def make(shape, azim, reg, kmax=3, **kw):
    return ref.problem(shape[0], shape[1], kmax, azim, reg[0], reg[1], seed=shape[0] * 100 + shape[1] + 7 * azim, **kw)


@pytest.mark.parametrize("reg", ref.REGS, ids=ref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_two_forms_agree_and_bounds_hold(case, reg):
    (nx, ny), azim = case
    prob = make((nx, ny), azim, reg)
    ng = (3 if azim else 1) * (nx - 2) * (ny - 2)
    sel = np.arange(ng)
    a, b = ref.linalg(prob, sel), ref.route(prob, sel)
    assert a["n_failed"] == b["n_failed"] == 0
    for k, v in ref.worst(b, a).items():
        assert v <= 1e-10, (k, v)
    for D, L, nd in ref.groups(prob):
        assert np.linalg.cond(ref.normal_matrix(prob, D, L)) <= 1e6
    nd = np.array([g[2] for g in ref.groups(prob)])
    assert (a["std_noise"] <= a["std_post"] * (1 + 1e-12)).all()
    tr = a["trace"].sum(axis=0)
    assert (tr >= -1e-12).all() and (tr < nd).all()
    if azim:
        assert (a["leak"] >= 0).all() and (a["leak"] <= 1).all()
    else:
        assert a["leak"] is None
    if reg[0] == 0.0:
        assert (a["rdiag"] >= -1e-12).all() and (a["rdiag"] < 1).all()
    if prob["dead"] is not None and reg[0] == 0.0:           # damping alone: a cell without rays resolves nothing, prior std 1 / damp
        j, i = divmod(prob["dead"], nx - 2)
        assert np.allclose(a["rdiag"][:, :, j, i], 0.0, atol=1e-14) and np.allclose(a["std_post"][:, :, j, i], 1 / prob["damp"])


@pytest.mark.parametrize("azim", [False, True], ids=["iso", "joint"])
def test_rows_are_the_solves_resolution(azim):
    """noise-free data d = G z of a true model z, solved by the dense normal equations with the regulariser: x = Rm z per period"""
    prob = make((9, 5), azim, (0.7, 0.3))
    ng = (3 if azim else 1) * 21
    want = ref.linalg(prob, np.arange(ng))
    rng = np.random.default_rng(5)
    for p, (D, L, _) in enumerate(ref.groups(prob)):
        z = rng.normal(size=ng)
        x = np.linalg.solve(ref.normal_matrix(prob, D, L), D @ z)   # G^T W^2 (G z) = D z
        assert np.abs(x - want["rows"][p] @ z).max() <= 1e-10 * max(1.0, np.abs(x).max())


def test_singular_period_is_nan_in_both_forms():
    prob = make((9, 5), False, (0.8, 0.0), no_reg_period=1)
    for fn in (ref.linalg, ref.route):
        out = fn(prob, np.array([0, 3]))
        assert out["n_failed"] == 1
        for k in ref.OUTPUTS:
            if out[k] is None:
                continue
            a = np.moveaxis(out[k], 0 if k == "rows" else 1, 0)
            assert np.isnan(a[1]).all() and np.isfinite(a[[0, 2]]).all(), k


def test_laplacian_rule():
    r, c, v = ref.laplacian2d(6, 5, [0.5, 2.0])
    ncell = 12
    A = np.zeros((2 * ncell, 2 * ncell))
    A[r, c] = v
    assert A[0, 0] == 1.0 and A[ncell + 3, ncell + 3] == 4.0
    inner = 1 * 4 + 1                                        # cell (j 1, i 1)
    assert A[inner, inner] == 2.0 and sorted(np.flatnonzero(A[inner])) == [inner - 4, inner - 1, inner, inner + 1, inner + 4]
    assert A[inner].sum() == 0.0 and not A[:ncell, ncell:].any() and not A[ncell:, :ncell].any()
