"""CPU: the long-row problems of tests/test_long_rows_gpu.py (model_posterior_ref.long_rows, map_posterior_ref.long_rows and the
right-hand sides of the two trade-off references) -- that they hold the rows they are made for, that their normal matrices are as well
conditioned as those the GPU bars were measured on (cond <= 1e4 at every regulariser, sweep point and P_k), and that the references
the GPU results are held to move by at least 100 bars when a row walk stops after one or two passes: the comparison is not blind to
what it is written for.
Measured: model cond(A_n) 2.13e2 at most, over the sweeps cond(A_k) 4.62e2 and cond(P_k) 1.81e3; maps cond(A_g) 8.12e1, over the
sweeps cond(A) 2.23e2 and cond(P) 2.78e3.  The change of the output that moves most, smallest over the cases: model 1.28e-1 behind 256
entries and 1.19e-2 behind 512; maps 9.72e-2 behind 64, 2.80e-2 behind 128 and 1.16e-2 behind 8 entries of the regularisation rows
(100 bars are 1e-4)."""
import functools

import numpy as np
import pytest

from tests import map_posterior_ref as pref
from tests import map_tradeoff_ref as ptref
from tests import model_posterior_ref as mref
from tests import model_tradeoff_ref as mtref

BAR = 1e-6            # the bar of the four GPU test modules
BLIND = 100 * BAR     # what a truncated row walk must move the reference by
MODES = [False, True]
MODEL_IDS, MAP_IDS = ["iso", "joint"], ["iso", "azim"]
ONE_DAMP = (1.0,)     # the sweep of the GPU tests: the five scales (and the Gc/Gs-only ones) at the problem's damping


@functools.lru_cache(maxsize=None)
def model_case(joint, reg):
    return mref.long_case(joint, reg)


@functools.lru_cache(maxsize=None)
def map_case(azim, reg, through_dead=False):
    return pref.long_case(azim, reg, through_dead=through_dead)


def check_triplets(prob):
    """1-based, sorted by (row, column), columns distinct inside a row, no empty row"""
    row, col = prob["irow"].astype(np.int64), prob["icol"].astype(np.int64)
    assert row.min() == 1 and row.max() == prob["m"] and col.min() >= 1 and col.max() <= prob["n"]
    key = row * (prob["n"] + 1) + col
    assert (np.diff(key) > 0).all()
    assert len(np.unique(row)) == prob["m"] and prob["rw"].dtype == np.float32


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("joint", MODES, ids=MODEL_IDS)
def test_model_census(joint, reg):
    """every length of the issue among the data rows and among the regularisation rows, exactly; the added data rows avoid the dead
    cell and span the blocks, the added regularisation rows stay inside one; the hub column has at least 129 data rows (three strides
    of 64 over a column of the transpose); neither row count is a multiple of 16 (MT_RG rows a wavefront)"""
    prob = model_case(joint, reg)
    base = mref.problem(*mref.LONG_SHAPES[joint], joint, reg[0], reg[1], seed=0)
    nvx, nvy, nlay, nblk, ncell, n = mref.dims(prob)
    assert n == (840 if joint else 550) == prob["n"]
    check_triplets(prob)
    nd, nr = len(mref.LONG_DATA), len(mref.LONG_REG[joint])
    assert prob["m_data"] == base["m_data"] + nd and prob["m"] == base["m"] + nd + nr
    dl, rl = mref.row_lengths(prob)
    assert tuple(dl[-nd:]) == mref.LONG_DATA and tuple(rl[-nr:]) == mref.LONG_REG[joint]
    assert dl[:-nd].max() <= 90 and (len(rl) == nr or rl[:-nr].max() <= 7)
    assert set(mref.LONG_LENS) <= set(dl) and set(mref.LONG_REG_SHORT) <= set(rl)
    assert set(l for l in mref.LONG_LENS if l <= (257 if joint else 513)) <= set(rl)
    row, col = prob["irow"].astype(np.int64) - 1, prob["icol"].astype(np.int64) - 1
    data = row < prob["m_data"]
    assert not (col[data] % ncell == prob["dead"]).any()
    added = (row >= prob["m_data"] - nd) & data
    assert set(col[added] // (ncell * nlay)) == set(range(nblk))
    assert np.abs(prob["rw"][added]).max() <= 3 / np.sqrt(255)
    L = mref.parts(prob)[1]
    assert len(mtref.blocks(prob, L)) == len(rl) and (mtref.blocks(prob, L) >= 0).all()       # (a row in two blocks is its assertion)
    per_col = np.bincount(col[data], minlength=n)
    print(f"\n[measured] data rows of the hub column {per_col[prob['hub']]}, of the next {np.sort(per_col)[-2]}")
    assert per_col[prob["hub"]] >= 129 and per_col.argmax() == prob["hub"]
    assert prob["m_data"] % 16 and len(rl) % 16


@pytest.mark.parametrize("reg", pref.REGS, ids=pref.REG_IDS)
@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_map_census(azim, reg):
    """every length of the issue among the data rows and among the regularisation rows of every period, exactly; the added data rows
    avoid the dead cell and span the blocks, every row stays inside one period and every regularisation row inside one block (the
    assertions of map_tradeoff_ref.periods); period 0 has 257 regularisation rows or more (a second batch of MP_TB = 256 in k_mp_rows)
    and more than 64 data rows; neither count is a multiple of 16 or 64.
    No column of a map has 129 data rows: six rows of each length per period are 42, and `problem`'s rows put about 8 on a cell.  No
    map kernel walks a column; their counterpart, the 64 rows of a ballot round, is test_map_column_behind_the_first_ballot_round."""
    prob = map_case(azim, reg)
    nx, ny = pref.LONG_SHAPES[azim]
    ncell, nblk, kmax = (nx - 2) * (ny - 2), 3 if azim else 1, pref.LONG_KMAX
    assert nblk * ncell == 210 and prob["n"] == 210 * kmax
    check_triplets(prob)
    dl, rl = mref.row_lengths(prob)
    row, col = prob["irow"].astype(np.int64) - 1, prob["icol"].astype(np.int64) - 1
    per_of_row = np.zeros(prob["m"], np.int64)
    per_of_row[row] = (col % (kmax * ncell)) // ncell
    parts = ptref.periods(dict(prob, b=np.zeros(prob["m_data"], np.float32)))
    for p, part in enumerate(parts):
        d, r = dl[per_of_row[:prob["m_data"]] == p], rl[per_of_row[prob["m_data"]:] == p]
        assert len(d) == len(part["G"]) and len(r) == len(part["L"])
        assert sorted(d[d > 18]) == sorted(l for l in pref.LONG_DATA_LENS for _ in range(6)) and set(pref.LONG_DATA_LENS) <= set(d)
        assert set(pref.LONG_REG_LENS) <= set(r) <= set(pref.LONG_REG_LENS) | {1, 5}
        assert len(d) > 64
    data = row < prob["m_data"]
    assert not (col[data] % ncell == prob["dead"]).any()
    long_data = data & (np.concatenate([dl, rl])[row] > 18)
    assert set(col[long_data] // (kmax * ncell)) == set(range(nblk))
    nd0, nr0 = len(parts[0]["G"]), len(parts[0]["L"])
    print(f"\n[measured] period 0: {nd0} data rows, {nr0} regularisation rows")
    assert nr0 >= pref.LONG_REG_ROWS
    assert nd0 % 16 and nd0 % 64 and nr0 % 16 and nr0 % 64


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("joint", MODES, ids=MODEL_IDS)
def test_model_condition(joint, reg):
    """a condition, not a measurement: the GPU bar of 1e-6 is the project's for this arithmetic at cond <= 1e4"""
    prob = model_case(joint, reg)
    cond = np.linalg.cond(mref.normal_matrix(prob, *mref.parts(prob)))
    print(f"\n[measured] cond(A_n) {cond:.2e}")
    assert cond <= mref.COND_MAX


@pytest.mark.parametrize("reg", pref.REGS, ids=pref.REG_IDS)
@pytest.mark.parametrize("through_dead", [False, True], ids=["", "through-dead"])
@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_map_condition(azim, through_dead, reg):
    prob = map_case(azim, reg, through_dead)
    cond = max(np.linalg.cond(pref.normal_matrix(prob, D, L)) for D, L, _ in pref.groups(prob))
    print(f"\n[measured] cond(A_g) {cond:.2e}")
    assert cond <= ptref.COND_MAX


@functools.lru_cache(maxsize=None)
def model_sweep(joint):
    prob = mtref.long_case(joint, mref.REGS[0])
    scale, damp = mtref.sweep(prob, ONE_DAMP)
    return prob, scale, damp, mtref.linalg(prob, scale, damp)


@functools.lru_cache(maxsize=None)
def map_sweep(azim, through_dead=False):
    prob = ptref.long_case(azim, pref.REGS[0], through_dead=through_dead)
    scale, damp = ptref.sweep(prob, ONE_DAMP)
    return prob, scale, damp, ptref.linalg(prob, scale, damp)


@pytest.mark.parametrize("joint", MODES, ids=MODEL_IDS)
def test_model_sweep_condition(joint):
    """every point of the GPU test's sweep: cond(A_k) and cond(P_k) <= 1e4, GCV's denominator away from 0; the point the dof
    comparison uses is there"""
    prob, scale, damp, out = model_sweep(joint)
    assert len(damp) == (10 if joint else 5) and (scale[2] == 1).all() and damp[2] == np.float32(prob["damp"])
    D, L = mref.parts(prob)
    blk = mtref.blocks(prob, L)
    assert not out["n_failed"].any()
    ca = cp = 0.0
    for k in range(len(damp)):
        P = mtref.prior(prob, L, blk, scale[k], damp[k])
        assert mtref.is_pd(P)
        ca, cp = max(ca, np.linalg.cond(D + P)), max(cp, np.linalg.cond(P))
    print(f"\n[measured] cond(A_k) {ca:.2e} cond(P_k) {cp:.2e}")
    assert ca <= mtref.COND_MAX and cp <= mtref.COND_MAX
    assert ((prob["m_data"] - out["dof"].sum(axis=1)) / prob["m_data"] >= 0.1).all()
    assert abs(out["dof"][2].sum() - mref.linalg(prob)["trace"].sum()) <= 1e-10 * prob["n"]


@pytest.mark.parametrize("through_dead", [False, True], ids=["", "through-dead"])
@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_map_sweep_condition(azim, through_dead):
    prob, scale, damp, out = map_sweep(azim, through_dead)
    nblk = 3 if azim else 1
    assert len(damp) == (10 if azim else 5) and (scale[2] == 1).all() and damp[2] == np.float32(prob["damp"])
    assert not out["n_failed"].any()
    ca = cp = 0.0
    for part in ptref.periods(prob):
        D = part["G"].T @ part["G"]
        for k in range(len(damp)):
            P = ptref.prior(part, nblk, scale[k], damp[k])
            assert ptref.is_pd(P)
            ca, cp = max(ca, np.linalg.cond(D + P)), max(cp, np.linalg.cond(P))
    slack = ((out["mdata_p"][None, :] - out["dof"].sum(axis=2)) / out["mdata_p"][None, :]).min()
    print(f"\n[measured] cond(A) {ca:.2e} cond(P) {cp:.2e} (m_p - dof)/m_p {slack:.3f}")
    assert ca <= ptref.COND_MAX and cp <= ptref.COND_MAX and slack >= 0.05
    assert np.abs(out["dof"][2].T - pref.linalg(prob)["trace"]).max() <= 1e-10 * 210


def spread(n):
    return np.unique(np.array([0, 1, n // 3, n // 2, n - 2, n - 1], np.int32))


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("keep", [256, 512])
@pytest.mark.parametrize("joint", MODES, ids=MODEL_IDS)
def test_model_posterior_reference_sees_the_later_passes(joint, keep, reg):
    """in the reference only, every row loses what stands behind its first `keep` entries (joint mode has no regularisation row and
    no pass behind 512 but the data rows')"""
    prob = model_case(joint, reg)
    sel = spread(prob["n"])
    moved = mref.worst(mref.linalg(mref.truncated(prob, keep), sel), mref.linalg(prob, sel))
    print(f"\n[measured] behind {keep}: {moved}")
    assert max(moved.values()) >= BLIND


@pytest.mark.parametrize("keep", [256, 512])
@pytest.mark.parametrize("joint", MODES, ids=MODEL_IDS)
def test_model_tradeoff_reference_sees_the_later_passes(joint, keep):
    prob, scale, damp, out = model_sweep(joint)
    moved = mtref.worst(mtref.linalg(mref.truncated(prob, keep), scale, damp), out)
    print(f"\n[measured] behind {keep}: {moved}")
    assert max(moved.values()) >= BLIND


MAP_CUTS = [(64, False), (128, False), (8, True)]
MAP_CUT_IDS = ["behind-64", "behind-128", "reg-behind-8"]


@pytest.mark.parametrize("reg", pref.REGS, ids=pref.REG_IDS)
@pytest.mark.parametrize("keep,reg_only", MAP_CUTS, ids=MAP_CUT_IDS)
@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_map_posterior_reference_sees_the_later_strides(azim, keep, reg_only, reg):
    """in the reference only, every row loses what stands behind its first 64 or 128 entries, and every regularisation row what stands
    behind its first MP_EMAX = 8"""
    prob = map_case(azim, reg)
    sel = spread(210)
    moved = pref.worst(pref.linalg(mref.truncated(prob, keep, reg_only), sel), pref.linalg(prob, sel))
    print(f"\n[measured] {'regularisation rows ' if reg_only else ''}behind {keep}: {moved}")
    assert max(moved.values()) >= BLIND


@pytest.mark.parametrize("keep,reg_only", MAP_CUTS, ids=MAP_CUT_IDS)
@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_map_tradeoff_reference_sees_the_later_strides(azim, keep, reg_only):
    prob, scale, damp, out = map_sweep(azim)
    moved = ptref.worst(ptref.linalg(mref.truncated(prob, keep, reg_only), scale, damp), out)
    print(f"\n[measured] {'regularisation rows ' if reg_only else ''}behind {keep}: {moved}")
    assert max(moved.values()) >= BLIND


@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_map_column_behind_the_first_ballot_round(azim):
    """through_dead: `problem` sends no data row through the dead cell, and every period has more than 64 of its rows (143 or 423),
    all in front of the added ones, so the dead cell's columns stand only in rows 64 and later of a period's list -- in a later
    round of the 64-row ballot of mp_rows_with (mp_accum_rows, the maps' k_mt_rhs).  Without those entries the references move by 100 bars and more."""
    prob, scale, damp, out = map_sweep(azim, True)
    nx, ny = pref.LONG_SHAPES[azim]
    ncell, nblk, kmax = (nx - 2) * (ny - 2), 3 if azim else 1, pref.LONG_KMAX
    row, col = prob["irow"].astype(np.int64) - 1, prob["icol"].astype(np.int64) - 1
    on_dead = (col % ncell == prob["dead"]) & (row < prob["m_data"])
    for p in range(kmax):
        in_p = (col % (kmax * ncell)) // ncell == p
        rows_p = np.unique(row[in_p & (row < prob["m_data"])])               # the period's data rows as its list has them
        for b in range(nblk):
            at = np.searchsorted(rows_p, np.unique(row[on_dead & in_p & (col // (kmax * ncell) == b)]))
            assert len(at) >= 42 // nblk and at.min() >= 64 and len(rows_p) > 64
    cut = dict(prob, irow=prob["irow"][~on_dead], icol=prob["icol"][~on_dead], rw=prob["rw"][~on_dead])
    sel = spread(210)
    assert pref.worst(pref.linalg(cut, sel), pref.linalg(prob, sel))["rdiag"] >= BLIND
    moved = ptref.worst(ptref.linalg(cut, scale, damp), out)
    print(f"\n[measured] without the dead cell's data entries: {moved}")
    assert moved["x"] >= BLIND and moved["dof"] >= BLIND
