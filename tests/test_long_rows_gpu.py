"""-m gpu: dazim_model_posterior, dazim_map_posterior, dazim_model_tradeoff and dazim_map_tradeoff on rows longer than one pass of
their row walks (the problems of model_posterior_ref.long_rows and map_posterior_ref.long_rows, which
tests/test_long_rows_ref_cpu.py takes the census, the condition and the sensitivity of).

model: data and regularisation rows of 255 .. 513 entries about the 256 of a pass of mo_accum_row (k_mo_gram, k_mt_gram_data,
k_mt_combine), a column of the transpose with more than 128 data rows (k_mt_rhs), row counts that are no multiple of the 16 rows of a
wavefront (k_mt_rows); these are tradeoff.hip's kernels over its view MtModel.  maps: data rows of 63 .. 200 entries about the strides
of 64 of mp_accum_rows and of the row search mp_rows_with under it (k_mp_gram, and k_mt_combine and k_mt_rhs over the view MtPeriod),
regularisation rows of 7 .. 66 entries about the MP_EMAX = 8 of k_mp_rows, 259 of them in period 0 (its second batch of
MP_TB = 256), a column that only rows of a later ballot round hold.  Against numpy.linalg at the bars of the four entries' own tests.

Tried on an MI355X with the walks cut short in the library: mo_accum_row after its first pass, mp_accum_rows' update or its search (and
the maps' k_mt_rhs's) after the first stride, k_mp_rows' long branch after 64 entries and its loop after the first batch.  Every test here fails
under the cuts its entry runs through (errors of 1e-4 .. 3e-1); of the 313 tests of the four entries' own modules one fails each time,
the synthetic survey's, whose rays are long enough."""
import functools

import numpy as np
import pytest

from tests import map_posterior_ref as pref
from tests import map_tradeoff_ref as ptref
from tests import model_posterior_ref as mref
from tests import model_tradeoff_ref as mtref
from tests import test_map_posterior_gpu as mp
from tests import test_map_tradeoff_gpu as mpt
from tests import test_model_posterior_gpu as mo
from tests import test_model_tradeoff_gpu as mt
from tests.bars import within

pytestmark = pytest.mark.gpu

MODES = [False, True]
MODEL_IDS, MAP_IDS = ["iso", "joint"], ["iso", "azim"]
ONE_DAMP = (1.0,)     # the sweep: the five scales (and the Gc/Gs-only, a1/a2-only ones) at the problem's damping; point 2 is scale 1


def frozen(prob):
    for a in prob.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return prob


def model_sel(prob):
    """the unknowns some_sel takes (first, a middle and the last chunk of 256 columns), their neighbours and the hub column"""
    n = prob["n"]
    return np.unique(np.append(mo.some_sel(n), [1, n - 2, prob["hub"]]).astype(np.int32))


def map_sel(prob):
    """the unknowns some_sel takes (first, a middle and the last stride of 64 columns), their neighbours and the dead cell of every block"""
    ng, ncell = mp.n_g(prob), prob["dead"] + 1
    return np.unique(np.concatenate([mp.some_sel(prob), [1, ng - 2], np.arange(ncell - 1, ng, ncell)]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def model_case(joint, reg):
    prob = frozen(mref.long_case(joint, reg))
    return prob, mref.linalg(prob, model_sel(prob))


@functools.lru_cache(maxsize=None)
def map_case(azim, reg, through_dead=False):
    prob = frozen(pref.long_case(azim, reg, through_dead=through_dead))
    return prob, pref.linalg(prob, map_sel(prob))


@functools.lru_cache(maxsize=None)
def model_sweep(joint):
    prob = frozen(mtref.long_case(joint, mref.REGS[0]))
    scale, damp = mtref.sweep(prob, ONE_DAMP)
    return prob, scale, damp, mtref.linalg(prob, scale, damp)


@functools.lru_cache(maxsize=None)
def map_sweep(azim, through_dead=False):
    prob = frozen(ptref.long_case(azim, pref.REGS[0], through_dead=through_dead))
    scale, damp = ptref.sweep(prob, ONE_DAMP)
    return prob, scale, damp, ptref.linalg(prob, scale, damp)


def plain_tiles(ctx, fn):
    ctx.set_option("map_post.mfma", 0)
    try:
        return fn()
    finally:
        ctx.set_option("map_post.mfma", 1)


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("joint", MODES, ids=MODEL_IDS)
def test_model_posterior_equals_numpy_linalg(ctx, joint, reg):
    """n = 550 and 840, twelve data rows and two regularisation rows of each of 255 .. 513 entries: every output within 1e-6 *
    max(1, max |reference|) of numpy.linalg, a second call the same bits; the plain tile form too at smooth+damp.
    Measured on an MI355X, largest over the 6 cases and both tile forms: 5.7e-8 (bar 1e-6)."""
    prob, want = model_case(joint, reg)
    sel = model_sel(prob)
    A = mo.matrix(ctx, prob)
    got = mo.call(ctx, A, prob, sel)
    assert got["n_failed"] == 0 and ctx.stat("model_post.n") == prob["n"]
    tag = f"{'joint' if joint else 'iso'} n {prob['n']}, long rows"
    big = 0.0
    for k, v in mref.worst(got, want).items():
        big = max(big, v)
        within(f"model_posterior vs numpy.linalg, {k}, {tag}", v, mo.BAR)
    mo.same_bits(mo.call(ctx, A, prob, sel), got, mref.OUTPUTS)
    if reg == mref.REGS[0]:
        for k, v in mref.worst(plain_tiles(ctx, lambda: mo.call(ctx, A, prob, sel)), want).items():
            big = max(big, v)
            within(f"model_posterior (plain tiles) vs numpy.linalg, {k}, {tag}", v, mo.BAR)
    print(f"\n[measured] {tag}: largest error against numpy.linalg {big:.3e}")
    A.free()


@pytest.mark.parametrize("reg", pref.REGS, ids=pref.REG_IDS)
@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_map_posterior_equals_numpy_linalg(ctx, azim, reg):
    """n_g = 210 at two periods, six data rows of each of 63 .. 200 entries per period, regularisation rows of 7 .. 66 entries, 259
    regularisation rows in period 0: every output within 1e-6 * max(1, max |reference|) of numpy.linalg, a second call the same bits;
    the plain tile form too at smooth+damp.
    Measured on an MI355X, largest over the 6 cases and both tile forms: 5.4e-8 (bar 1e-6)."""
    prob, want = map_case(azim, reg)
    sel = map_sel(prob)
    A = mp.matrix(ctx, prob)
    got = mp.call(ctx, A, prob, sel)
    assert got["n_failed"] == 0
    tag = f"{'azim' if azim else 'iso'} n_g {mp.n_g(prob)}, long rows"
    big = 0.0
    for k, v in pref.worst(got, want).items():
        big = max(big, v)
        within(f"map_posterior vs numpy.linalg, {k}, {tag}", v, mp.BAR)
    mp.same_bits(mp.call(ctx, A, prob, sel), got, pref.OUTPUTS)
    if reg == pref.REGS[0]:
        for k, v in pref.worst(plain_tiles(ctx, lambda: mp.call(ctx, A, prob, sel)), want).items():
            big = max(big, v)
            within(f"map_posterior (plain tiles) vs numpy.linalg, {k}, {tag}", v, mp.BAR)
    print(f"\n[measured] {tag}: largest error against numpy.linalg {big:.3e}")
    A.free()


@pytest.mark.parametrize("joint", MODES, ids=MODEL_IDS)
def test_model_tradeoff_equals_numpy_linalg_and_dof_is_the_trace(ctx, joint):
    """the same problems with a right-hand side at smooth+damp, over the five scales at the problem's damping (joint: and on the
    Gc/Gs blocks alone): every output within the bar of numpy.linalg, a second call the same bits, the plain tile form in joint mode;
    at scale 1 dof per block is dazim_model_posterior's trace -- k_mt_combine adds what k_mo_gram adds, pass by pass.
    Measured on an MI355X, largest of both cases: 3.5e-8, dof against the trace 1.9e-8 (bar 1e-6)."""
    prob, scale, damp, want = model_sweep(joint)
    A = mt.matrix(ctx, prob)
    got = mt.call(ctx, A, prob, scale, damp)
    assert not got["n_failed"].any() and ctx.stat("model_trade.n") == prob["n"] and ctx.stat("model_trade.points") == len(damp)
    tag = f"{'joint' if joint else 'iso'} n {prob['n']}, long rows"
    big = 0.0
    for k, v in mtref.worst(got, want).items():
        big = max(big, v)
        within(f"model_tradeoff vs numpy.linalg, {k}, {tag}", v, mt.BAR)
    mt.same_bits(mt.call(ctx, A, prob, scale, damp), got)
    if joint:
        for k, v in mtref.worst(plain_tiles(ctx, lambda: mt.call(ctx, A, prob, scale, damp)), want).items():
            big = max(big, v)
            within(f"model_tradeoff (plain tiles) vs numpy.linalg, {k}, {tag}", v, mt.BAR)
    assert (scale[2] == 1).all() and damp[2] == np.float32(prob["damp"])
    post = mo.call(ctx, A, prob)
    A.free()
    per_block = np.asarray(post["trace"], np.float64).sum(axis=1)
    tr = float(per_block.sum())
    within(f"model_tradeoff sum of dof vs model_posterior's trace, {tag}", abs(got["dof"][2].sum() - tr) / max(1.0, abs(tr)), mt.BAR)
    within(f"model_tradeoff dof per block vs model_posterior's trace per block, {tag}",
           np.abs(got["dof"][2] - per_block).max() / max(1.0, per_block.max()), mt.BAR)
    print(f"\n[measured] {tag}: largest error against numpy.linalg {big:.3e}")


def map_tradeoff_against_linalg(ctx, azim, through_dead, plain):
    prob, scale, damp, want = map_sweep(azim, through_dead)
    A = mpt.matrix(ctx, prob)
    got = mpt.call(ctx, A, prob, scale, damp)
    assert not got["n_failed"].any() and ctx.stat("map_trade.ng") == 210 and ctx.stat("map_trade.points") == len(damp)
    assert ctx.stat("map_trade.grams") == prob["kmax"] and np.array_equal(got["mdata_p"], want["mdata_p"])
    tag = f"{'azim' if azim else 'iso'} n_g 210, long rows{', through the dead cell' if through_dead else ''}"
    big = 0.0
    for k, v in ptref.worst(got, want).items():
        big = max(big, v)
        within(f"map_tradeoff vs numpy.linalg, {k}, {tag}", v, mpt.BAR)
    for k, v in mtref.worst(got["total"], ptref.totals(want), ptref.TOTALS).items():
        big = max(big, v)
        within(f"map_tradeoff totals vs numpy, {k}, {tag}", v, mpt.BAR)
    mpt.same_bits(mpt.call(ctx, A, prob, scale, damp), got)
    if plain:
        for k, v in ptref.worst(plain_tiles(ctx, lambda: mpt.call(ctx, A, prob, scale, damp)), want).items():
            big = max(big, v)
            within(f"map_tradeoff (plain tiles) vs numpy.linalg, {k}, {tag}", v, mpt.BAR)
    assert (scale[2] == 1).all() and damp[2] == np.float32(prob["damp"])
    post = mp.call(ctx, A, prob)
    A.free()
    tr = np.asarray(post["trace"], np.float64)              # [nblk][kmax]
    dof = got["dof"][2].T                                    # [nblk][kmax]
    within(f"map_tradeoff sum of dof per period vs map_posterior's trace, {tag}",
           np.abs(dof.sum(axis=0) - tr.sum(axis=0)).max() / max(1.0, tr.sum(axis=0).max()), mpt.BAR)
    within(f"map_tradeoff dof per block and period vs map_posterior's trace, {tag}", np.abs(dof - tr).max() / max(1.0, tr.max()), mpt.BAR)
    print(f"\n[measured] {tag}: largest error against numpy.linalg {big:.3e}")


@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_map_tradeoff_equals_numpy_linalg_and_dof_is_the_trace(ctx, azim):
    """the same problems with a right-hand side at smooth+damp, over the five scales at the problem's damping (azim: and on the
    a1/a2 blocks alone): every output and total within the bar of numpy.linalg, a second call the same bits, the plain tile form
    with azim; at scale 1 dof per block and period is dazim_map_posterior's trace -- k_mt_combine<MtPeriod> adds what k_mp_gram adds, stride
    by stride.
    Measured on an MI355X, largest of both cases: 4.5e-8, dof against the trace 3.0e-8 (bar 1e-6)."""
    map_tradeoff_against_linalg(ctx, azim, False, azim)


@pytest.mark.parametrize("azim", MODES, ids=MAP_IDS)
def test_a_column_only_later_ballot_rounds_hold(ctx, azim):
    """map_posterior_ref.long_rows with through_dead: every added data row holds the dead cell's column of one block.  `problem`
    sends no data row through that cell and gives every period more than 64 rows (423 and 143 here), all of them in front of the
    added ones in the period's list: the column stands only in rows 64 and later, which mp_accum_rows and the maps' k_mt_rhs reach in their
    second round of 64 rows or later (tests/test_long_rows_ref_cpu.py asserts the positions).  The dead cells are in sel.
    Measured on an MI355X, largest of both cases and both entries: 4.9e-8, dof against the trace 3.5e-8 (bar 1e-6)."""
    prob, want = map_case(azim, pref.REGS[0], True)
    sel = map_sel(prob)
    assert {b * (prob["dead"] + 1) + prob["dead"] for b in range(3 if azim else 1)} <= set(sel)
    A = mp.matrix(ctx, prob)
    got = mp.call(ctx, A, prob, sel)
    A.free()
    assert got["n_failed"] == 0
    big = 0.0
    for k, v in pref.worst(got, want).items():
        big = max(big, v)
        within(f"map_posterior vs numpy.linalg, {k}, {'azim' if azim else 'iso'}, through the dead cell", v, mp.BAR)
    print(f"\n[measured] {'azim' if azim else 'iso'}, through the dead cell: largest error of map_posterior against numpy.linalg {big:.3e}")
    map_tradeoff_against_linalg(ctx, azim, True, False)
