"""CPU: the fp64 restatement of the radial column problem (tests/column_radial_ref.py) holds: with no coupling it is the isotropic
restatement block by block, its resolution matrix is C blockdiag(Kv^T Wv^2 Kv, Kh^T Wh^2 Kh) and is the solve's, and the plan of the
kernel (packed lower triangle, potrf -> trtri -> lauum in place) gives what numpy.linalg gives, so that a GPU failure can be told
from a weakness of the plan itself.  Bar: the column solve's own, 1e-6 * max(1, max |reference|) per cell and output."""
import numpy as np
import pytest

from tests import column_radial_ref as ref
from tests.bars import within
from tests.test_column_lsq_gpu import lsq_numpy

NX, NY = 7, 6
NCELL = (NX - 2) * (NY - 2)
REGS = [(0.7, 0.3), (0.0, 0.5), (0.8, 0.0)]
REG_IDS = ["smooth+damp", "damp", "smooth"]


@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("kv,kh", [(1, 1), (16, 7), (4, 0), (0, 4)])
@pytest.mark.parametrize("nlay", [1, 2, 11])
def test_without_coupling_it_is_the_isotropic_restatement_per_block(nlay, kv, kh, reg):
    kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = ref.radial_problem(NX, NY, nlay, kv, kh, seed=nlay * 100 + kv + kh)
    x, ne, st = ref.per_cell_solve(NX, NY, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0, *reg, 0.0)
    assert ne >= 1 and not x[:, :, 3].any()
    off = 0
    for blk, (kern, rhs, w) in enumerate(((kern_v, rhs_v, w_v), (kern_h, rhs_h, w_h))):
        if kern is None:
            assert np.abs(x[blk]).max() <= 1e-12             # (lstsq's rounding; the kernel gives 0 exactly)
            continue
        xb, stb = lsq_numpy(NX, NY, nlay, kern, rhs[None], w, *reg)
        within(f"block {blk} vs lsq_numpy, nlay {nlay} kv {kv} kh {kh}", np.abs(x[blk] - xb[0]).max() / max(1.0, np.abs(xb).max()), 1e-9)
        assert np.allclose(st[off:off + kern.shape[1]], stb[0], rtol=1e-9, atol=0)
        off += kern.shape[1]


@pytest.mark.parametrize("couple", [0.0, 0.7, 50.0])
@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("kv,kh", [(1, 1), (16, 7), (3, 0)])
def test_resolution_matrix_is_c_times_the_data_matrix_and_is_the_solves(kv, kh, reg, couple):
    """Rm = C blockdiag(Kv^T Wv^2 Kv, Kh^T Wh^2 Kh) = I - C P2, and x = Rm x_true for noise-free data with d0 = 0"""
    nlay = 6
    kern_v, kern_h, _, _, w_v, w_h, _ = ref.radial_problem(NX, NY, nlay, kv, kh, seed=kv * 10 + kh)
    rng = np.random.default_rng(3)
    for c in (0, 5, 7, 11):
        Kv, wv = ref.cell_slices(NX, NY, nlay, kern_v, w_v, c)
        Kh, wh = ref.cell_slices(NX, NY, nlay, kern_h, w_h, c)
        one = ref.linalg(Kv, wv, Kh, wh, *reg, couple)
        C = np.linalg.inv(ref.data_matrix(Kv, wv, Kh, wh) + ref.penalty2(nlay, *reg, couple))
        P2 = ref.penalty2(nlay, *reg, couple)
        within(f"C N vs I - C P2, cell {c}", np.abs(one["rows"] - (np.eye(2 * nlay) - C @ P2)).max(), 1e-9 * max(1.0, np.abs(C).max() * np.abs(P2).max()))
        z = rng.standard_normal(2 * nlay)
        x = ref.solve(Kv, wv, Kv @ z[:nlay], Kh, wh, Kh @ z[nlay:], np.zeros(nlay), *reg, couple)
        within(f"solve(K z) vs Rm z, cell {c}", np.abs(x - one["rows"] @ z).max(), 1e-9 * max(1.0, np.abs(C).max()))


@pytest.mark.parametrize("couple", [0.0, 0.7, 50.0])
@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("kv,kh", [(1, 0), (0, 1), (1, 1), (16, 7), (30, 30)])
@pytest.mark.parametrize("nlay", [1, 2, 3, 11])
def test_the_kernels_plan_equals_linalg(nlay, kv, kh, reg, couple):
    kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = ref.radial_problem(NX, NY, nlay, kv, kh, seed=nlay * 100 + kv + kh)
    got = ref.per_cell_res(ref.route, NX, NY, nlay, kern_v, kern_h, w_v, w_h, *reg, couple)
    want = ref.per_cell_res(ref.linalg, NX, NY, nlay, kern_v, kern_h, w_v, w_h, *reg, couple)
    assert got["n_empty"] == want["n_empty"] >= 1 and got["n_failed"] == 0
    for k, v in ref.worst(got, want).items():
        within(f"route vs linalg, {k}, nlay {nlay} kv {kv} kh {kh} couple {couple}", v, 1e-6)


def test_the_kernels_plan_beyond_one_wavefront():
    """N = 66 on one cell: the posterior and the solution of the normal equations against linalg and the stacked lstsq"""
    nlay, kv, kh = 33, 16, 7
    kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0 = ref.radial_problem(NX, NY, nlay, kv, kh, seed=9)
    Kv, wv = ref.cell_slices(NX, NY, nlay, kern_v, w_v, 0)
    Kh, wh = ref.cell_slices(NX, NY, nlay, kern_h, w_h, 0)
    got, want = ref.route(Kv, wv, Kh, wh, 0.7, 0.3, 0.7), ref.linalg(Kv, wv, Kh, wh, 0.7, 0.3, 0.7)
    for k in ref.OUTPUTS:
        within(f"route vs linalg, {k}, one cell at nlay 33", np.abs(got[k] - want[k]).max() / max(1.0, np.abs(want[k]).max()), 1e-6)
    rv, rh, d = rhs_v.reshape(kv, -1)[:, 0].astype(float), rhs_h.reshape(kh, -1)[:, 0].astype(float), d0.reshape(nlay, -1)[:, 0].astype(float)
    m2 = ref.f32(0.7) ** 2
    b = np.concatenate([Kv.T @ (wv * wv * rv) + m2 * d, Kh.T @ (wh * wh * rh) - m2 * d])
    x = ref.route(Kv, wv, Kh, wh, 0.7, 0.3, 0.7, rhs=b)
    xs = ref.solve(Kv, wv, rv, Kh, wh, rh, d, 0.7, 0.3, 0.7)
    within("normal equations vs stacked lstsq, one cell at nlay 33", np.abs(x.astype(np.float32) - xs).max() / max(1.0, np.abs(xs).max()), 1e-6)


def test_known_problem_by_hand():
    """one knot, one period each: A = [[a + m, -m], [-m, h + m]] with a = wv^2 kv^2 + d^2, h likewise"""
    Kv, wv, Kh, wh = np.array([[3.0]]), np.array([2.0]), np.array([[1.0]]), np.array([0.5])
    d2, m2 = 0.25, ref.f32(0.7) ** 2
    A = np.array([[36.0 + d2 + m2, -m2], [-m2, 0.25 + d2 + m2]])
    C = np.linalg.inv(A)
    for fn in (ref.route, ref.linalg):
        o = fn(Kv, wv, Kh, wh, 0.0, 0.5, 0.7)
        assert np.allclose(o["std"], np.sqrt(np.diag(C))) and np.isclose(o["cov_vh"][0], C[0, 1])
        assert np.allclose(o["rdiag"], [C[0, 0] * 36.0, C[1, 1] * 0.25]) and np.allclose(o["trace"], o["rdiag"])
        assert np.allclose(o["cross"], [C[0, 1] * 0.25 / (C[0, 0] * 36.0 + C[0, 1] * 0.25), C[1, 0] * 36.0 / (C[1, 0] * 36.0 + C[1, 1] * 0.25)])
    x = ref.solve(Kv, wv, np.array([1.0]), Kh, wh, np.array([2.0]), np.array([0.1]), 0.0, 0.5, 0.7)
    assert np.allclose(x, C @ np.array([4.0 * 3.0 * 1.0 + m2 * 0.1, 0.25 * 1.0 * 2.0 - m2 * 0.1]))


def test_route_reports_a_failed_factorisation():
    kern_v, kern_h, _, _, w_v, w_h, _ = ref.radial_problem(NX, NY, 3, 4, 4, seed=2)
    kern_h = kern_h.copy()
    p = int(np.flatnonzero(w_h.reshape(4, -1)[:, 0])[0])  # a Love period of cell 0 that has data
    kern_h[1, p, 1 * NX + 1] = np.nan
    got = ref.per_cell_res(ref.route, NX, NY, 3, kern_v, kern_h, w_v, w_h, 0.7, 0.3, 0.7)
    assert got["n_failed"] == 1 and np.isnan(got["std"][:, 0]).all() and np.isfinite(got["std"][:, 1:]).all()
