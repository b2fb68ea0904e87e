"""-m gpu: the resident matrix (dazim_csr) through its life cycle.  Beside rowptr / col / val the matrix carries derived state --
the transpose, the 16-bit column copy, the column-block pointers, vmax, split_row / long_avg, the reserved capacities -- and
every mutation of an outer iteration (row scaling, data weights, appended rows, the thresholded copy) repairs that state by hand.

The oracle needs no tolerance: no product reads the capacities and every dispatch input is recomputed from the content, the
scatter form adds integers and the blocked form combines its partials in a fixed order, so after ANY sequence of mutations the
matrix G must behave like F = csr_from_coo(to_coo(G)) built afterwards: aprod(1), aprod(2), col_abs_sums and a 10-iteration
LSMR (x and info) return the same bits on both.  Beside it every state is compared with a NumPy model (tests/matrix_model.py):
to_coo exactly, both products with an fp64 scipy product under the bars of test_sparse_gpu.py (rel-L2 <= 2e-6 below 2^22 entries,
<= 3e-6 at the large shapes), col_abs_sums under the bound its arithmetic gives (see `check`).

Before every mutation both products have run on G, so every cache exists when it is mutated."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests.bars import within
from tests.matrix_model import Model
from tests.test_outer_iteration_gpu import cal_ddat_sigma, tikhonov_coo

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSMR_CFG = (0.01, 1e-9, 1e-9, 1e8, 10, 5)      # damp, atol, btol, conlim, itnlim = 10, localSize: ten iterations, no stop before


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def products(ctx, A, x, y):
    """(A x, A^T y) from zero vectors"""
    y1 = np.zeros(A.m, f32); ctx.aprod(1, A, x, y1)
    x2 = np.zeros(A.n, f32); ctx.aprod(2, A, x2, y)
    return y1, x2


def warm(ctx, G):
    """both products on G: afterwards every cache a product builds on first use (the transpose of the gather form) exists"""
    products(ctx, G, np.ones(G.n, f32), np.ones(G.m, f32))


def rel_l2(a, ref):
    nr = np.linalg.norm(ref)
    return np.linalg.norm(a.astype(np.float64) - ref) / nr if nr > 0 else float(np.abs(a).max(initial=0.0))


def check(ctx, G, model, where, large=False):
    """G against the model and against a matrix built afresh from G's own triplets"""
    assert (G.m, G.n, G.nnz) == (model.m, model.n, model.nnz), where
    ir, ic, rw = G.to_coo()
    mr, mc, mv = model.coo()
    assert np.array_equal(ir, mr) and np.array_equal(ic, mc), where
    assert np.array_equal(bits(rw), bits(mv)), where
    rng = np.random.default_rng(model.nnz + 7 * model.m)
    x = rng.standard_normal(G.n).astype(f32)
    y = rng.standard_normal(G.m).astype(f32)
    b = rng.standard_normal(G.m).astype(f32)
    F = ctx.csr_from_coo(G.m, G.n, ir, ic, rw)
    try:
        # -- a mutated matrix is indistinguishable from a fresh one
        yg, xg = products(ctx, G, x, y)
        yf, xf = products(ctx, F, x, y)
        assert np.array_equal(bits(yg), bits(yf)), f"{where}: A x differs from the fresh matrix's"
        assert np.array_equal(bits(xg), bits(xf)), f"{where}: A^T y differs from the fresh matrix's"
        dg, df = G.col_abs_sums(), F.col_abs_sums()
        assert np.array_equal(bits(dg), bits(df)), f"{where}: col_abs_sums differs from the fresh matrix's"
        sg, ig = ctx.lsmr(G, b, *LSMR_CFG)
        sf, jf = ctx.lsmr(F, b, *LSMR_CFG)
        assert np.array_equal(bits(sg), bits(sf)), f"{where}: LSMR x differs from the fresh matrix's"
        assert ig["istop"] == jf["istop"] and ig["itn"] == jf["itn"], (where, ig, jf)
        keys = ("normA", "condA", "normr", "normAr", "normx")
        assert np.array_equal(bits([ig[k] for k in keys]), bits([jf[k] for k in keys])), (where, ig, jf)
    finally:
        F.free()
    # -- and it is the model's matrix
    S = model.csr64()
    bar = 3e-6 if large else 2e-6
    assert large == (model.nnz >= 1 << 22)
    within(f"{where}: A x rel-L2 vs fp64", rel_l2(yg, S @ x.astype(np.float64)), bar)
    within(f"{where}: A^T y rel-L2 vs fp64", rel_l2(xg, S.T @ y.astype(np.float64)), bar)
    # col_abs_sums adds round-to-nearest(|v| * 2^(40 - e)) as integers, vmax < 2^e <= 2 vmax (m < 2^22: 40 fractional bits), and
    # rounds the sum to fp32 once: at most half a quantum 2^(e-40) <= vmax 2^-39 per entry, and 2^-24 relative
    assert model.m < 1 << 22
    a = np.abs(model.vals.astype(np.float64))
    ref = np.bincount(model.cols, weights=a, minlength=model.n)
    k = np.bincount(model.cols, minlength=model.n)
    vmax = a.max(initial=0.0)
    bound = 2.0 ** -24 * ref + k * vmax * 2.0 ** -40
    err = np.abs(dg.astype(np.float64) - ref)
    print(f"\n[measured] {where}: col_abs_sums max err/bound {np.max(err[bound > 0] / bound[bound > 0], initial=0.0):.3f}")
    assert (err <= bound).all(), (where, float(np.max(err - bound)))
    if model.nnz:
        assert dg.max() > 0


def random_rows(rng, m, n, lo, hi):
    """m rows of lo..hi entries, distinct ascending columns, no zero value"""
    cnt = rng.integers(lo, hi + 1, m)
    rows = np.repeat(np.arange(m), cnt)
    cols = np.concatenate([np.sort(rng.choice(n, c, replace=False)) for c in cnt])
    vals = rng.standard_normal(len(rows)).astype(f32)
    vals[vals == 0] = f32(1.0)
    return rows, cols, vals


def data(rng, n):
    """observed and synthetic times with outliers (the exp() branch of CalDdatSigma), as test_outer_iteration_gpu.py draws them"""
    obst = (20 + 80 * rng.random(n)).astype(f32)
    dsyn = (obst * (1 + 0.02 * rng.standard_normal(n))).astype(f32)
    dsyn[::17] *= f32(1.08)
    return obst, dsyn


def weight_data_step(ctx, G, model, dall, rng):
    """weight_data on the first dall rows: the weights are CalDdatSigma's (under the bar test_outer_iteration_gpu.py holds them
    to: the device's exp may round the other way on a tie), the rows of G times the weights returned, one fp32 product each"""
    obst, dsyn = data(rng, dall)
    res, wgt, rhs, st = ctx.weight_data(G, obst, dsyn)
    res_o = (obst - dsyn).astype(f32)
    sig, mean, sd = cal_ddat_sigma(obst, res_o)
    w_o = (f32(1) / sig).astype(f32)
    assert np.array_equal(res, res_o) and st["meandeltaT"] == float(mean) and st["stddeltaT"] == float(sd)
    assert np.array_equal(wgt, w_o) or np.abs(wgt / w_o - 1).max() <= 1.2e-7
    model.scale_rows(wgt, nrows=dall)


# the small grid: three blocks of 7 * 6 * 4 = 168 columns
NX, NY, NZ, WEIGHTS = 9, 8, 5, [2.0, 0.5, 1.25]
MAXVP = (NX - 2) * (NY - 2) * (NZ - 1)
NCOL = 3 * MAXVP
NRAY = 300


def ray_model(seed=11):
    rng = np.random.default_rng(seed)
    return Model(NRAY, NCOL, *random_rows(rng, NRAY, NCOL, 6, 40)), rng


def upload(ctx, model, reserve=None):
    """the model on the device: from COO (no room: every append reallocates) or, reserve = (rows, entries), its threshold(0) copy
    with that much room behind it"""
    G = ctx.csr_from_coo(model.m, model.n, *model.coo())
    if reserve is None:
        return G
    R = G.threshold(0.0, reserve[0], reserve[1])
    G.free()
    return R


@pytest.mark.parametrize("capacity", ["none", "exact", "one_short"])
def test_small_sequence(ctx, capacity):
    """every mutation of an outer iteration in turn on one matrix (gather kernels): where every append reallocates, where exactly
    enough room was reserved for all of them (in place), and with one entry too few (the last append falls back)"""
    model, rng = ray_model()
    shares = [(0, 51), (51, 2 * MAXVP), (2 * MAXVP, 3 * MAXVP)]      # (51 lies between two seven-entry rows)
    extra = random_rows(rng, 5, NCOL, 3, 12)
    tikh_nnz = len(tikhonov_coo(NX, NY, NZ, 0, WEIGHTS)[3])
    reserve = {"none": None, "exact": (3 * MAXVP + 5, tikh_nnz + len(extra[2])),
               "one_short": (3 * MAXVP + 5, tikh_nnz + len(extra[2]) - 1)}[capacity]
    G = upload(ctx, model, reserve)
    check(ctx, G, model, "built")
    # 1. scale_rows (with the transpose present)
    w = (rng.random(G.m) + 0.5).astype(f32)
    G.scale_rows(w); model.scale_rows(w)
    check(ctx, G, model, "scale_rows")
    # 2. weight_data over all rows
    warm(ctx, G)
    weight_data_step(ctx, G, model, G.m, rng)
    check(ctx, G, model, "weight_data")
    # 3. the Tikhonov rows in three consecutive shares
    for lo, hi in shares:
        warm(ctx, G)
        G.append_tikhonov_rows(NX, NY, NZ, WEIGHTS, lo, hi); model.append_tikhonov_rows(NX, NY, NZ, WEIGHTS, lo, hi)
        check(ctx, G, model, f"share [{lo}, {hi})")
    # 4. scale_rows over all rows, tail included; a few rows shrink below the threshold of step 7
    warm(ctx, G)
    w = (rng.random(G.m) + 0.5).astype(f32)
    w[5:NRAY:23] = f32(2e-5); w[NRAY + 3::41] = f32(1e-5)
    G.scale_rows(w); model.scale_rows(w)
    check(ctx, G, model, "scale_rows with tail")
    # 5. weight_data on the data rows only: the tail stays bit-identical (the model leaves it alone)
    warm(ctx, G)
    tail = G.to_coo()[2][model.rows >= NRAY]
    weight_data_step(ctx, G, model, NRAY, rng)
    assert np.array_equal(bits(G.to_coo()[2][model.rows >= NRAY]), bits(tail))
    check(ctx, G, model, "weight_data with tail")
    # 6. a few more rows as COO, handed over in another order than the matrix keeps
    warm(ctx, G)
    perm = rng.permutation(len(extra[2]))
    G.append_coo(5, (extra[0][perm] + G.m + 1).astype(np.int32), (extra[1][perm] + 1).astype(np.int32), extra[2][perm])
    model.append(5, *extra)
    check(ctx, G, model, "append_coo")
    # 7. the thresholded copy with room for one more block of regularisation rows
    warm(ctx, G)
    T = G.threshold(1e-4, 3 * MAXVP, tikh_nnz)
    tmodel = model.threshold(1e-4)
    assert 0 < tmodel.nnz < model.nnz
    check(ctx, T, tmodel, "threshold")
    check(ctx, G, model, "threshold: the source")
    # 8. on the copy, an in-place append
    warm(ctx, T)
    T.append_tikhonov(NX, NY, NZ, WEIGHTS); tmodel.append_tikhonov_rows(NX, NY, NZ, WEIGHTS)
    check(ctx, T, tmodel, "threshold + append_tikhonov")
    T.free(); G.free()


# shares of the 504 regularisation rows: a cut between two seven-entry rows (51), one at a block boundary (168), the empty share,
# a one-row share, a share spanning two blocks with different weights
SHARES = [(0, 51), (51, MAXVP), (MAXVP, MAXVP), (MAXVP, MAXVP + 1), (MAXVP + 1, 400), (400, 3 * MAXVP)]


@pytest.mark.parametrize("in_place", [False, True])
def test_share_geometry(ctx, in_place):
    """each share alone behind the same ray rows is that slice of the full block of tikhonov_coo; put together they are
    append_tikhonov"""
    base, _ = ray_model(5)
    cnt, tr, tc, tw = tikhonov_coo(NX, NY, NZ, 0, WEIGHTS)
    order = np.lexsort((tc, tr))
    tr, tc, tw = tr[order] - 1, tc[order] - 1, tw[order]
    assert cnt == 3 * MAXVP and SHARES[0][0] == 0 and SHARES[-1][1] == cnt
    assert all(a[1] == b[0] for a, b in zip(SHARES, SHARES[1:]))
    assert len(tw[tr == 50]) == 7 and len(tw[tr == 51]) == 7
    reserve = (cnt, len(tw)) if in_place else None
    for lo, hi in SHARES:
        model = base.copy()
        G = upload(ctx, model, reserve)
        warm(ctx, G)
        x = np.linspace(-1, 1, G.n).astype(f32); y = np.linspace(1, 2, G.m).astype(f32)
        before = products(ctx, G, x, y)
        G.append_tikhonov_rows(NX, NY, NZ, WEIGHTS, lo, hi)
        sel = (tr >= lo) & (tr < hi)
        model.append(hi - lo, tr[sel] - lo, tc[sel], tw[sel])
        check(ctx, G, model, f"share [{lo}, {hi}) alone")
        if lo == hi:
            assert (G.m, G.nnz) == (base.m, base.nnz)
            after = products(ctx, G, x, y)
            assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(before, after))
        G.free()
    G, W = upload(ctx, base, reserve), upload(ctx, base, reserve)
    for lo, hi in SHARES:
        warm(ctx, G)
        G.append_tikhonov_rows(NX, NY, NZ, WEIGHTS, lo, hi)
    W.append_tikhonov(NX, NY, NZ, WEIGHTS)
    for p, q in zip(G.to_coo(), W.to_coo()):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))
    model = base.copy()
    model.append(cnt, tr, tc, tw)
    check(ctx, G, model, "all shares")
    G.free(); W.free()


def test_refused_appends_leave_the_matrix_alone(ctx):
    model, _ = ray_model(6)
    G = upload(ctx, model, (3 * MAXVP, 4000))
    warm(ctx, G)
    x = np.linspace(-1, 1, G.n).astype(f32); y = np.linspace(1, 2, G.m).astype(f32)
    before = products(ctx, G, x, y)
    bad = {"row_lo < 0": (NX, NY, NZ, WEIGHTS, -1, 5),
           "row_hi < row_lo": (NX, NY, NZ, WEIGHTS, 5, 3),
           "row_hi > nblock * maxvp": (NX, NY, NZ, WEIGHTS, 0, 3 * MAXVP + 1),
           "nblock = 65": (3, 3, 2, [1.0] * 65, 0, 65),                 # (one cell per block: the 65 blocks fit the columns)
           "blocks wider than n": (NX, NY, NZ, WEIGHTS + [1.0], 0, 10)}
    for name, args in bad.items():
        with pytest.raises(dz.DazimError) as e:
            G.append_tikhonov_rows(*args)
        assert e.value.code == dz.DAZIM_E_BAD_ARG, name
        assert (G.m, G.nnz) == (model.m, model.nnz), name
        after = products(ctx, G, x, y)
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(before, after)), name
        check(ctx, G, model, f"refused: {name}")
    G.free()


@pytest.mark.parametrize("in_place", [False, True])
def test_matrix_without_entries(ctx, in_place):
    """m >= 1 rows and no entry, then an append: the rebuild of every derived array from entry 0"""
    model = Model(4, NCOL, [], [], np.zeros(0, f32))
    tikh_nnz = len(tikhonov_coo(NX, NY, NZ, 0, WEIGHTS)[3])
    G = upload(ctx, model, (3 * MAXVP, tikh_nnz) if in_place else None)
    check(ctx, G, model, "no entries")
    for lo, hi in ((0, 100), (100, 3 * MAXVP)):
        warm(ctx, G)
        G.append_tikhonov_rows(NX, NY, NZ, WEIGHTS, lo, hi); model.append_tikhonov_rows(NX, NY, NZ, WEIGHTS, lo, hi)
        check(ctx, G, model, f"no entries + share [{lo}, {hi})")
    G.free()


@pytest.mark.parametrize("in_place", [False, True])
def test_laplacian2d_append(ctx, in_place):
    """the maps' 2-D regularisation rows (append_laplacian2d) behind rows that carry every cache, then a row scaling"""
    nx, ny, w = 12, 9, [1.5, 0.75, 2.0, 3.0, 0.5, 1.25]
    ncell = (nx - 2) * (ny - 2)
    rng = np.random.default_rng(8)
    model = Model(150, len(w) * ncell, *random_rows(rng, 150, len(w) * ncell, 6, 40))
    reg = Model(0, model.n, [], [], np.zeros(0, f32))
    reg.append_laplacian2d(nx, ny, w)
    G = upload(ctx, model, (reg.m, reg.nnz) if in_place else None)
    warm(ctx, G)
    G.append_laplacian2d(nx, ny, w); model.append_laplacian2d(nx, ny, w)
    check(ctx, G, model, "laplacian2d")
    warm(ctx, G)
    s = (rng.random(G.m) + 0.5).astype(f32)
    G.scale_rows(s); model.scale_rows(s)
    check(ctx, G, model, "laplacian2d + scale_rows")
    G.free()


@pytest.mark.parametrize("nx,ny,nz,nblock,kind", [(40, 40, 17, 1, 1), (52, 52, 17, 1, 2), (52, 52, 17, 3, 2)])
def test_production_layout(ctx, nx, ny, nz, nblock, kind):
    """>= 2^22 entries in long rows, then the 1- and 7-entry regularisation tail appended in place in three shares: the smallest
    shapes that select A x with the whole x in LDS (n = 23 104), blocked with the 16-bit column itself (n = 40 000) and blocked with
    16-bit columns relative to the block pair (n = 120 000 > 65 536); A^T y in the scatter form throughout.  8191 rows of 521
    entries: the appended entries start at 4 267 511, not a multiple of the four entries a narrowing step handles"""
    import torch
    num_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    maxvp = (nx - 2) * (ny - 2) * (nz - 1)
    n, m, per_row = nblock * maxvp, 8191, 521
    assert m * per_row >= 1 << 22 and (m * per_row) % 4 != 0 and m >= 16 * num_cu
    rng = np.random.default_rng(n)
    start = rng.integers(0, n, m)
    cols = (start[:, None] + np.cumsum(rng.integers(1, 6, (m, per_row)), axis=1)) % n
    cols.sort(axis=1)
    vals = (-np.abs(rng.standard_normal(m * per_row)) * 0.2 - 1e-3).astype(f32)
    model = Model(m, n, np.repeat(np.arange(m), per_row), cols.reshape(-1), vals)
    weights = [2.0, 0.5, 1.25][:nblock]
    nreg = nblock * maxvp
    reg = Model(0, n, [], [], np.zeros(0, f32))
    reg.append_tikhonov_rows(nx, ny, nz, weights)
    G = upload(ctx, model, (nreg, reg.nnz))

    def dispatch(after_append):
        warm(ctx, G)
        # the whole-x LDS form needs 64 * num_cu rows, the blocked and scatter forms 16 * num_cu: the ray rows alone may be too few
        # for the first, the appended matrix has them
        want = kind if (kind == 2 or G.m >= 64 * num_cu) else 0
        assert not after_append or want == kind
        assert ctx.stat("spmv.kind") == want and ctx.stat("spmvt.kind") == 1
        assert ctx.stat("spmv.idx_bytes") == (2 if want else 4) and ctx.stat("spmvt.idx_bytes") == 2
        split = m if after_append else G.m
        assert ctx.stat("spmvt.split_row") == split and split <= G.m
        if kind == 2:
            assert ctx.stat("spmv.split_row") == split
    dispatch(False)
    check(ctx, G, model, "ray rows", large=True)
    cuts = [0, nreg // 3 + 1, nreg - 7, nreg]
    for lo, hi in zip(cuts, cuts[1:]):
        warm(ctx, G)
        G.append_tikhonov_rows(nx, ny, nz, weights, lo, hi); model.append_tikhonov_rows(nx, ny, nz, weights, lo, hi)
        if hi != cuts[2]:                              # (first and last share: four or five checks per shape)
            check(ctx, G, model, f"share [{lo}, {hi})", large=True)
    assert m < G.m
    dispatch(True)
    w = (rng.random(G.m) + 0.5).astype(f32)
    G.scale_rows(w); model.scale_rows(w)
    dispatch(True)
    check(ctx, G, model, "scale_rows", large=True)
    G.free()


@pytest.mark.parametrize("world", [2, 3])
def test_weights_sharded_over_ranks(ctx, tmp_path, world):
    """dazim_weight_data_sharded over real ranks (tests/weights_shard_worker.py): uneven slices of one list of 20 877 data (not a
    multiple of the 8192-entry chunk of the sequential sums) put together are the one-rank call bit for bit"""
    from tests.weights_shard_worker import CUTS, problem
    obst, dsyn, model = problem()
    dall = len(obst)
    G = ctx.csr_from_coo(model.m, model.n, *model.coo())
    res1, wgt1, rhs1, st1 = ctx.weight_data(G, obst, dsyn)
    rw1 = G.to_coo()[2]
    G.free()
    comm_dir = tmp_path / "comm"
    comm_dir.mkdir()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "weights_shard_worker.py"), str(r), str(world), str(comm_dir),
                               str(tmp_path / f"out{r}.npz")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[-2000:] for o in outs]
    parts = [np.load(tmp_path / f"out{r}.npz") for r in range(world)]
    cuts = CUTS[world]
    assert cuts[0] == 0 and cuts[-1] == dall and len(set(np.diff(cuts))) == world
    for r, d in enumerate(parts):
        assert (int(d["row0"]), int(d["dall"])) == (cuts[r], cuts[r + 1] - cuts[r])
        assert np.array_equal(bits(d["xt"]), bits(d["xt_fresh"])) and np.abs(d["xt"]).max() > 0, r
    for name, one in (("res", res1), ("wgt", wgt1), ("rhs", rhs1), ("rw", rw1)):
        assert np.array_equal(bits(np.concatenate([d[name] for d in parts])), bits(one)), name
    keys = list(st1)
    for r, d in enumerate(parts):
        st = dict(zip(keys, d["stats"]))
        for k in ("meandeltaT", "stddeltaT"):
            assert bits(st[k]) == bits(st1[k]), (r, k)
        for k in ("mean", "std", "mean_abs", "rms", "mean_weight", "mean_abs_weighted"):
            # the ranks add the same doubles in another order: only the final rounding to fp32 can move
            assert abs(float(st[k]) - st1[k]) <= float(np.spacing(f32(abs(st1[k])))), (r, k, float(st[k]), st1[k])
            assert bits(st[k]) == bits(dict(zip(keys, parts[0]["stats"]))[k]), (r, k)     # (one all-reduced sum: the same on every rank)
    assert sorted(os.listdir(comm_dir)) == []
