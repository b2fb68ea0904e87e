"""-m gpu: every form of A x and A^T y, col_abs_sums and to_coo against int64 sums, bit for bit, on the matrices of
tests/spmv_cases.py: integer values and vectors make every summation order exact, so there is no tolerance anywhere in this file.
The cases plant the edges of the row walk (tests/test_spmv_cases_cpu.py counts them); the forms that ran are read back from the
library's statistics and compared with the model's prediction.  Non-finite values: DESIGN.md section 5."""
import numpy as np
import pytest

from tests import spmv_cases as sc

pytestmark = pytest.mark.gpu
f32 = np.float32
FAST = ("spmv.ldsx", "spmv.blocked", "spmv.scatter")


def num_cu(ctx):
    import torch
    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def same_bits(got, want_int, what):
    want = np.asarray(want_int).astype(f32)
    assert np.array_equal(want.astype(np.int64), want_int), what          # the reference itself is exact in fp32
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} differ, first at {bad[:8]}: {got[bad[:8]]} instead of {want[bad[:8]]}"


def upload(ctx, case):
    return ctx.csr_from_coo(case.m, case.n, case.irow, case.icol, case.rw)


def check_products(ctx, A, case, what):
    """aprod(1) and aprod(2), from zeros and onto integer vectors"""
    ref = case.refs
    y = np.zeros(case.m, f32); ctx.aprod(1, A, case.x.copy(), y)
    same_bits(y, ref["Ax"], f"{case.name}, {what}: A x")
    y = case.y0.copy(); ctx.aprod(1, A, case.x.copy(), y)
    same_bits(y, ref["Ax"] + case.y0.astype(np.int64), f"{case.name}, {what}: y0 + A x")
    x = np.zeros(case.n, f32); ctx.aprod(2, A, x, case.y.copy())
    same_bits(x, ref["ATy"], f"{case.name}, {what}: A^T y")
    x = case.x0.copy(); ctx.aprod(2, A, x, case.y.copy())
    same_bits(x, ref["ATy"] + case.x0.astype(np.int64), f"{case.name}, {what}: x0 + A^T y")


def ran(ctx):
    """the dispatch of the last A x and A^T y as the library recorded it (the split rows only of the forms that have them)"""
    d = {k: int(ctx.stat(s)) for k, s in (("spmv_kind", "spmv.kind"), ("spmv_lanes", "spmv.lanes"), ("spmv_idx", "spmv.idx_bytes"),
                                          ("spmvt_kind", "spmvt.kind"), ("spmvt_lanes", "spmvt.lanes"), ("spmvt_idx", "spmvt.idx_bytes"))}
    rows = set()
    if d["spmv_kind"] == 2:
        rows.add(int(ctx.stat("spmv.split_row")))
    if d["spmvt_kind"] == 1:
        rows.add(int(ctx.stat("spmvt.split_row")))
    return d, rows


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_exact(ctx, name):
    C = num_cu(ctx)
    case = sc.build(name, C)
    ax, aty = case.bounds()
    assert ax < 1 << 24 and aty < 1 << 24
    want = sc.dispatch(case, C)
    table = sc.EXPECT[name]
    assert {k: want[k] for k in table if k != "split"} == {k: table[k] for k in table if k != "split"}
    assert (want["split_row"] < case.m) == table["split"]
    A = upload(ctx, case)
    try:
        check_products(ctx, A, case, "default options")
        got, rows = ran(ctx)
        assert (int(ctx.stat("spmv.ncb")), int(ctx.stat("spmv.cbw"))) == (case.ncb, case.cbw)
        assert got == {k: want[k] for k in got}
        assert rows == {want["split_row"]}
        same_bits(A.col_abs_sums(), case.refs["colabs"], f"{name}: col_abs_sums")
        irow, icol, rw = A.to_coo()
        o = case.order
        assert np.array_equal(irow, case.irow[o]) and np.array_equal(icol, case.icol[o])
        assert np.array_equal(rw.view(np.uint32), case.rw[o].view(np.uint32))
        # one lane grouping for every row
        ctx.set_option("spmv.split", 0)
        check_products(ctx, A, case, "spmv.split = 0")
        got, rows = ran(ctx)
        flat = sc.dispatch(case, C, split=False)
        assert got == {k: flat[k] for k in got} and rows == {case.m}
        ctx.set_option("spmv.split", 1)
        # the gather forms
        for k in FAST:
            ctx.set_option(k, 0)
        check_products(ctx, A, case, "gather forms")
        got, _ = ran(ctx)
        assert got == dict(spmv_kind=0, spmv_lanes=0, spmv_idx=4, spmvt_kind=0, spmvt_lanes=0, spmvt_idx=4)
        for k in FAST:
            ctx.set_option(k, 1)
        # 32-bit column indices
        A.free()
        ctx.set_option("spmv.col16", 0)
        A = upload(ctx, case)
        ctx.set_option("spmv.col16", 1)
        check_products(ctx, A, case, "spmv.col16 = 0")
        got, rows = ran(ctx)
        assert got == {**{k: want[k] for k in got}, "spmv_idx": 4, "spmvt_idx": 4} and rows == {want["split_row"]}
    finally:
        for k in FAST + ("spmv.split", "spmv.col16"):
            ctx.set_option(k, 1)
        A.free()


# ---- non-finite values: A^T y leaves the fixed-point scatter form and both products propagate them ----

@pytest.fixture(scope="module")
def long64(ctx):
    """the case, the planted row that the tests poison (a few hundred distinct columns, the block-boundary ones among them), its
    columns and values"""
    case = sc.build("long64", num_cu(ctx))
    r = case.marks["wide"]
    rowptr, col = case.csr
    cols = col[rowptr[r]:rowptr[r + 1]]
    vals = case.rw[case.order][rowptr[r]:rowptr[r + 1]]
    assert len(cols) >= 300 and len(np.unique(cols)) == len(cols) and 0 in cols and case.n - 1 in cols
    return case, r, cols, vals


def scatter_first(ctx, A, case):
    """a finite A^T y first: the scatter form runs and says so, so that spmvt.kind = 0 afterwards is the doing of the next call"""
    x = np.zeros(case.n, f32); ctx.aprod(2, A, x, case.y.copy())
    same_bits(x, case.refs["ATy"], "finite A^T y")
    assert ctx.stat("spmvt.kind") == 1


def exact_except(got, want_int, at, what):
    """integers, bit for bit, everywhere but at the indices `at`; returns the values there"""
    keep = np.ones(len(got), bool); keep[at] = False
    same_bits(got[keep], np.asarray(want_int)[keep], what)
    return got[at]


def test_nan_in_y(ctx, long64):
    case, r, cols, vals = long64
    A = upload(ctx, case)
    try:
        scatter_first(ctx, A, case)
        y = case.y.copy(); y[r] = np.nan
        x = np.zeros(case.n, f32); ctx.aprod(2, A, x, y)
        yi = case.y.astype(np.int64); yi[r] = 0
        assert np.all(np.isnan(exact_except(x, case.S.T @ yi, cols, "A^T y beside the NaN row's columns")))
        assert ctx.stat("spmvt.kind") == 0
    finally:
        A.free()


def test_inf_in_y(ctx, long64):
    case, r, cols, vals = long64
    A = upload(ctx, case)
    try:
        scatter_first(ctx, A, case)
        y = case.y.copy(); y[r] = np.inf
        x = np.zeros(case.n, f32); ctx.aprod(2, A, x, y)
        yi = case.y.astype(np.int64); yi[r] = 0
        there = exact_except(x, case.S.T @ yi, cols, "A^T y beside the Inf row's columns")
        assert np.array_equal(there, np.sign(vals) * f32(np.inf))
        assert ctx.stat("spmvt.kind") == 0
    finally:
        A.free()


def test_nan_matrix_value(ctx, long64):
    case, r, cols, vals = long64
    A = upload(ctx, case)
    try:
        scatter_first(ctx, A, case)
        w = np.ones(case.m, f32); w[r] = np.nan
        A.scale_rows(w)
        y = np.zeros(case.m, f32); ctx.aprod(1, A, case.x.copy(), y)
        assert np.isnan(exact_except(y, case.refs["Ax"], [r], "A x beside the NaN row"))[0]
        x = np.zeros(case.n, f32); ctx.aprod(2, A, x, case.y.copy())
        yi = case.y.astype(np.int64); yi[r] = 0
        assert np.all(np.isnan(exact_except(x, case.S.T @ yi, cols, "A^T y beside the NaN row's columns")))
        assert ctx.stat("spmvt.kind") == 0
    finally:
        A.free()


def test_nan_in_x(ctx, long64):
    case, r, cols, vals = long64
    c = case.n - 1
    rows = np.unique(case.irow[case.icol == c + 1].astype(np.int64) - 1)
    assert r in rows and len(rows) > 64
    A = upload(ctx, case)
    try:
        xv = case.x.copy(); xv[c] = np.nan
        y = np.zeros(case.m, f32); ctx.aprod(1, A, xv, y)
        xi = case.x.astype(np.int64); xi[c] = 0
        assert np.all(np.isnan(exact_except(y, case.S @ xi, rows, "A x beside the rows that hold the NaN column")))
    finally:
        A.free()


def test_lsmr_nan_in_b(ctx, long64):
    """a NaN in b: ||b|| is NaN, every A^T u of the solve takes the gather form and the NaN reaches x instead of a finite, wrong
    solution.  The host loop enqueues at most itnlim iterations and then stops whatever the state says (LsmrSolve::run), so the
    call returns."""
    import dazimsurftomo_amd as dz
    case, r, cols, vals = long64
    A = upload(ctx, case)
    try:
        scatter_first(ctx, A, case)
        b = case.y.copy(); b[r] = np.nan
        x = np.zeros(case.n, f32)
        try:
            ctx.lsmr(A, b, 0.0, 1e-6, 1e-6, 1e8, 3, 0, x=x)
        except dz.DazimError:
            pass
        assert ctx.stat("spmvt.kind") == 0
        filled = case.refs["colabs"] > 0
        assert filled.sum() > case.n // 2
        assert not np.any(np.isfinite(x[filled]) & (x[filled] != 0))
    finally:
        A.free()
