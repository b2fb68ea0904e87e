"""The vectorised row generators of tests/matrix_model.py (the reference of tests/test_matrix_lifecycle_gpu.py at its large shapes)
against the loops that restate the reference statement by statement: `tikhonov_coo` and `lap2d_numpy` of the existing tests."""
import numpy as np
import pytest

from tests.matrix_model import Model, laplacian2d_rows, tikhonov_rows
from tests.test_outer_iteration_gpu import tikhonov_coo
from tests.test_phase_maps_gpu import lap2d_numpy

GRIDS = [(9, 8, 5, [2.0, 0.5, 1.25]), (5, 7, 3, [1.5]), (4, 4, 4, [3.0, 0.25]), (6, 5, 6, [0.1, 7.0, 7.0])]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("nx,ny,nz,weights", GRIDS)
def test_tikhonov_rows_equal_the_loop(nx, ny, nz, weights):
    cnt, ir, ic, rw = tikhonov_coo(nx, ny, nz, 0, weights)
    order = np.lexsort((ic, ir))                       # (the loop writes a stencil centre first, the device ascending columns)
    r, c, v = tikhonov_rows(nx, ny, nz, weights)
    assert cnt == (nx - 2) * (ny - 2) * (nz - 1) * len(weights)
    assert np.array_equal(r, ir[order] - 1) and np.array_equal(c, ic[order] - 1) and np.array_equal(bits(v), bits(rw[order]))
    # any share is that slice of the full block, rows counted from the share's first
    for lo, hi in ((0, 0), (3, 4), (cnt // 3, cnt - 2), (cnt - 1, cnt)):
        rs, cs, vs = tikhonov_rows(nx, ny, nz, weights, lo, hi)
        sel = (r >= lo) & (r < hi)
        assert np.array_equal(rs, r[sel] - lo) and np.array_equal(cs, c[sel]) and np.array_equal(bits(vs), bits(v[sel]))


@pytest.mark.parametrize("nx,ny,nz,weights", GRIDS)
def test_laplacian2d_rows_equal_the_loop(nx, ny, nz, weights):
    r0, c0, v0 = lap2d_numpy(nx, ny, weights)
    r, c, v = laplacian2d_rows(nx, ny, weights)
    assert np.array_equal(r, r0) and np.array_equal(c, c0) and np.array_equal(bits(v), bits(v0))


def test_model_mutations():
    """append, scaling of the leading rows only, threshold: on a matrix small enough to read"""
    M = Model(2, 4, [0, 0, 1], [1, 3, 0], np.array([1.0, -2.0, 1e-5], np.float32))
    M.append(1, [0], [2], np.array([4.0], np.float32))
    M.scale_rows(np.array([0.5, 3.0, 100.0], np.float32), nrows=2)
    f = np.float32
    assert M.m == 3 and np.array_equal(bits(M.vals), bits([f(0.5), f(-1.0), f(1e-5) * f(3.0), f(4.0)]))
    T = M.threshold(1e-4)
    assert (T.m, T.nnz) == (3, 3) and np.array_equal(T.rows, [0, 0, 2]) and np.array_equal(T.cols, [1, 3, 2])
    assert np.array_equal(M.csr64().toarray()[2], [0, 0, 4.0, 0])
