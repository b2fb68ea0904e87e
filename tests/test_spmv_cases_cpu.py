"""tests/spmv_cases.py on its own (no GPU): every case that tests/test_spmv_exact_gpu.py uploads holds the walk edges it was built
for -- counted from the built matrix, not assumed --, keeps every sum below 2^24, so that the int64 reference is what exact fp32
arithmetic gives, and selects the kernel forms of its row in the table, by the model of the dispatch that the GPU test compares
with the library's own statistics.  C = 256 compute units (MI355X) and one other value."""
import numpy as np
import pytest

from tests import spmv_cases as sc


@pytest.mark.parametrize("C", [256, 304])
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case(name, C):
    case = sc.build(name, C)
    # the shape: COO, 1-based, shuffled; integer values and vectors in range
    assert case.irow.min() >= 1 and case.irow.max() <= case.m and case.icol.min() == 1 and case.icol.max() == case.n
    assert np.any(np.diff(case.irow) < 0) and len(case.irow) == len(case.icol) == len(case.rw) == case.nnz
    assert set(np.unique(np.abs(case.rw)).tolist()) == set(range(1, 8))
    for v, k in ((case.x, case.n), (case.y, case.m), (case.x0, case.n), (case.y0, case.m)):
        assert v.dtype == np.float32 and len(v) == k and np.abs(v).min() >= 1 and np.abs(v).max() <= 8 and np.all(v == np.round(v))
    assert case.cbw == sc.block_width(case.n, case.ncb) and (case.ncb - 1) * case.cbw < case.n <= case.ncb * case.cbw
    # the planted classes
    assert sc.missing_classes(case, C) == []
    # exactness of the reference
    ax, aty = case.bounds()
    assert ax < 1 << 24 and aty < 1 << 24
    assert np.abs(case.refs["colabs"]).max() < 1 << 24
    # the dispatch
    d = sc.dispatch(case, C)
    want = sc.EXPECT[name]
    assert case.nnz >= sc.NNZ_MIN
    assert {k: d[k] for k in want if k != "split"} == {k: want[k] for k in want if k != "split"}
    assert (d["split_row"] < case.m) == want["split"]
    if want["split"]:
        assert d["split_row"] == case.marks["tail"]
    assert sc.dispatch(case, C, split=False)["split_row"] == case.m


def test_walk_parts():
    """the model of walk_rows' cut against a plain loop over small ranges"""
    for s in range(9):
        for e in range(s, s + 14):
            head, al, tail = (int(v) for v in sc.walk_parts(np.array([s]), np.array([e])))
            i, h = s, 0
            while i < e and i % 4:
                i += 1; h += 1
            a = (e - i) // 4 * 4
            assert (head, al, tail) == (h, a, e - i - a)


def test_split_rows():
    assert sc.split_rows(np.array([70, 3, 64, 5, 0])) == (3, 137 / 3)
    assert sc.split_rows(np.array([3, 5, 63])) == (3, 71 / 3)          # no long row
    assert sc.split_rows(np.array([3, 5, 64])) == (3, 72 / 3)          # the long row is last: no tail
