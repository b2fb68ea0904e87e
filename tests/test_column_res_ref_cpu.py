"""CPU: the route dazim_column_resolution takes (tests/column_res_ref.py: Cholesky, inverse factor by columns, C = M^T M,
Rm = I - C P) against numpy.linalg.inv(A) and inv(A) @ K^T W^2 K on the problems of the GPU test, so that a GPU failure can be told
from a weakness of the route itself.  Bar: the column solve's own, 1e-6 * max(1, max |reference|) per cell and output."""
import numpy as np
import pytest

from tests import column_res_ref as ref
from tests.bars import within
from tests.test_column_lsq_gpu import random_problem

NX, NY = 7, 6
REGS = [(0.7, 0.3), (0.0, 0.5), (0.8, 0.0)]
REG_IDS = ["smooth+damp", "damp", "smooth"]


def problem(nlay, kmax, fp32):
    kern, _, w = random_problem(NX, NY, nlay, kmax, 1, fp32, seed=nlay * 1000 + kmax * 10 + 1)
    return kern, w, ref.knot_depths(nlay)


@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kmax", [1, 4, 60])
@pytest.mark.parametrize("nlay", [1, 2, 3, 11, 63])
def test_route_equals_linalg(nlay, kmax, fp32, reg):
    kern, w, depz = problem(nlay, kmax, fp32)
    got = ref.per_cell(ref.route, NX, NY, nlay, kern, w, *reg, depz)
    want = ref.per_cell(ref.linalg, NX, NY, nlay, kern, w, *reg, depz)
    empty = ~(w.reshape(kmax, -1) != 0).any(axis=0)
    assert empty[3] and got["n_empty"] == want["n_empty"] == int(empty.sum()) and got["n_failed"] == 0
    for k, v in ref.worst(got, want).items():
        within(f"route vs linalg, {k}, nlay {nlay} kmax {kmax}", v, 1e-6)


def test_route_of_a_known_problem():
    """one knot, one period: A = w^2 k^2 + d^2, so C = 1 / A, Rm = w^2 k^2 / A and the noise variance Rm C, by hand"""
    K, w = np.array([[3.0]]), np.array([2.0])
    for fn in (ref.route, ref.linalg):
        o = fn(K, w, 0.0, 0.5, np.zeros(1, np.float32))
        A = 36.0 + 0.25
        assert np.isclose(o["std_post"][0], A ** -0.5) and np.isclose(o["rdiag"][0], 36.0 / A) and np.isclose(o["trace"], 36.0 / A)
        assert np.isclose(o["std_noise"][0], 6.0 / A) and np.isclose(o["rsum"][0], 36.0 / A) and o["width"][0] == 0.0


def test_route_reports_a_failed_factorisation():
    kern, w, _ = problem(3, 4, 0)
    kern = kern.copy()
    p = int(np.flatnonzero(w.reshape(4, -1)[:, 0])[0])    # a period of cell 0 that has data
    kern[1, p, 1 * NX + 1] = np.nan
    got = ref.per_cell(ref.route, NX, NY, 3, kern, w, 0.7, 0.3)
    assert got["n_failed"] == 1 and np.isnan(got["std_post"][:, 0]).all() and np.isfinite(got["std_post"][:, 1:]).all()
