"""CPU: the cases of tests/typed_cases.py reach what they are named for, and the yardstick that tests/test_disp_typed_shapes_gpu.py
holds dazim_dispersion_kernels_typed to is the reference's at these shapes too.

  reach    typed_cases.plan -- the host arithmetic of csrc/disp_typed.hip restated -- gives every case the layers, patch rows,
           items and columns per workgroup worked out by hand from the host code (typed_cases.EXPECTED), partial last
           workgroups, workgroups over several columns and, on 64 knots, columns over several workgroups.  The GPU test reads
           the items per workgroup back from the library (stat disp_typed.items_per_wg), which keeps this mirror honest.
  shares   the oracle-driven yardstick against the one driven by the reference subroutine (needs oracle/_ref), every case, under
           typed_kernels_ref.check_tables: the bars' shares C_SHARE, U_SHARE cap what a device test may leave out, and here the
           reference alone stays within them.  Measured: oracle and reference are bit-equal on every entry of every table of every
           case (190- and 197-layer stacks, 60 periods included).
  ended    where the Love curves of the falling columns end, and that the yardstick's depth kernels are 0 there."""
import numpy as np
import pytest

from oracle.pyoracle import Ref
from tests import typed_cases as TC
from tests import typed_kernels_ref as T

needs_ref = pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libdazim_ref.so not built")
CASES = TC.cases()


@pytest.fixture(scope="module")
def oracle_tables(orc):
    """{name: (pv, sen)} of the oracle-driven yardstick, computed lazily, once, and left alone"""
    cache = {}

    def get(name):
        if name not in cache:
            pv, sen = TC.tables(CASES[name], orc.surfdisp96_full)
            for a in (pv,) + tuple(sen or ()):
                a.setflags(write=False)
            cache[name] = (pv, sen)
        return cache[name]
    return get


# ---- reach ----
def test_the_mirror_on_the_common_model():
    """what the issue states for the model every earlier test runs on: 64 items and 5 columns per workgroup, patch 8, 17 layers"""
    p = TC.plan(T.DEPZ, T.SUBLAYERS, T.SEGMENTS, True, T.NX * T.NY)
    assert (p.mmax, p.npatch, p.tw, p.cpb) == (17, 8, 64, 5)
    assert p.typed == [1, 2, 3] and p.nvar == [31, 21, 21] and p.blocks == [10, 7, 7] and p.lds <= TC.LDS_MAX
    assert TC.plan(T.DEPZ, T.SUBLAYERS, T.SEGMENTS, False, T.NX * T.NY).tw == 64       # 5 knots: curves only still runs 64


@pytest.mark.parametrize("name", list(TC.EXPECTED))
def test_plan_of_the_case(name):
    c, p = CASES[name], TC.case_plan(CASES[name])
    print(f"\n[{name}] mmax {p.mmax} npatch {p.npatch} tw {p.tw} cpb {p.cpb} lds {p.lds} nvar {p.nvar} blocks {p.blocks} last {p.last}")
    assert (p.mmax, p.npatch, p.tw, p.cpb) == TC.EXPECTED[name]
    assert c["vel"].shape == (len(c["depz"]), c["ny"], c["nx"]) and p.mmax <= TC.NL and p.lds <= TC.LDS_MAX
    if name in TC.EXPECTED_BLOCKS:
        assert (p.blocks, p.last) == TC.EXPECTED_BLOCKS[name]
    # one halving earlier the tables do not fit: tw is the loop's choice, not a smaller one
    if p.tw < TC.TW:
        nvar_min, tw = min(p.nvar), 2 * p.tw
        cpb = (tw + nvar_min - 1) // nvar_min + 1
        assert (8 * p.mmax + 4 * cpb * p.mmax + 3 * p.npatch * tw + 3 * cpb * p.nz) * 4 > TC.LDS_MAX


@pytest.mark.parametrize("name", list(CASES))
def test_work_split_of_the_case(name):
    c, p = CASES[name], TC.case_plan(CASES[name])
    assert all(0 < n < p.tw for n in p.last), "a last workgroup that is empty or full"
    spans = [[b - a + 1 for a, b in TC.columns_of_workgroups(p, g)] for g in range(len(p.typed))]
    assert max(max(s) for s in spans) <= p.cpb                     # (cpb is what a workgroup may span)
    if name == "one_column":
        assert p.ncol == 1 and p.cpb > 1                           # base tables 1 .. cpb - 1 have no column
    else:
        assert all(max(s) >= 2 for s in spans), "no workgroup over two columns"
    if name == "two_knots":
        assert max(spans[1]) == 8 and p.cpb == 9
    if name == "max_knots":
        for g in range(3):
            per_col = [TC.workgroups_of_column(p, g, col) for col in range(p.ncol)]
            assert [b - a + 1 for a, b in per_col] == ([7, 7] if g == 0 else [5, 5])
            assert per_col[0][1] == per_col[1][0]                  # one workgroup: the tail of column 0, the head of column 1
    if name == "np60":
        assert all(len(t) == TC.NP for _, _, t in c["segments"])
    if c["kernels"] and c["falling"] is not None and p.ncol > 1:   # the falling column's variants lie in two workgroups (Love)
        for g in (1, 2):
            a, b = TC.workgroups_of_column(p, g, c["falling"])
            assert b == a + 1
    if not c["kernels"]:
        assert p.nvar == [1, 1, 1] and p.cpb == p.tw + 1
        if c["falling"] is not None:
            assert c["falling"] == (p.blocks[0] - 1) * p.tw      # the first item of the last workgroup


def test_the_boundary_pair_pins_the_loop_from_both_sides():
    """curves only on 2 knots: mmax = sublayers + 2, and the loop keeps 64 items while 4 (8 m + 4 x 65 m + 3 x 65 x 2) <= 64 KiB,
    i.e. m <= 59"""
    (s64, m64), (s32, m32) = TC.boundary_sublayers()
    assert m32 == m64 + 1 and s32 == s64 + 1
    lo, hi = TC.case_plan(CASES["curves_tw64_last"]), TC.case_plan(CASES["curves_tw32_first"])
    assert (lo.mmax, lo.tw, lo.cpb) == (m64, 64, 65) and (hi.mmax, hi.tw, hi.cpb) == (m32, 32, 33)
    assert lo.lds <= TC.LDS_MAX < lo.lds + 4 * (8 + 4 * 65)        # one layer more does not fit at 64 items
    assert m64 == 59


def test_curves_only_runs_below_64_items_from_15_knots():
    """the fallback is the normal case for curves only: at sublayers 3 (4 nz - 3 layers) 13 knots still run 64 items per
    workgroup, 14 .. 25 run 32 (4 x 659 nz <= 64 KiB + 4 x 420), 26 .. 46 run 16, 47 .. 50 run 8"""
    tw = {nz: TC.plan(3.0 * np.arange(nz), 3.0, TC.SEGMENTS, False, 70).tw for nz in range(2, 51)}
    first = {t: min(nz for nz in tw if tw[nz] == t) for t in (32, 16, 8)}
    print(f"\n[curves only, sublayers 3] first knot count at 32 / 16 / 8 items per workgroup: {first}")
    assert tw[13] == 64 and first == {32: 14, 16: 26, 8: 47} and tw[15] == 32 and tw[30] == 16 and tw[50] == 8
    assert all(TC.plan(3.0 * np.arange(nz), 3.0, TC.SEGMENTS, True, 70).tw == 64 for nz in (15, 30))    # with depth kernels: 64


def test_refused_shapes():
    """64 knots at sublayers 3: 253 layers > NL, which the host refuses before it plans"""
    assert len(TC.refine_layers(2.0 * np.arange(64), 3.0)) == 253 > TC.NL


# ---- shares ----
@needs_ref
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_driven_yardstick_against_the_reference_driven_one(oracle_tables, name):
    c = CASES[name]
    want = TC.tables(c, Ref().surfdisp96_full)
    T.check_tables(f"{name}: oracle vs reference", oracle_tables(name), want, c["vel"], c["segments"])
    assert (want[0] != 0).mean() >= 0.75                           # (not a comparison of zeros; one_column: 2 of 8 ended)


# ---- ended curves ----
@pytest.mark.parametrize("name", list(CASES))
def test_where_the_love_curves_of_the_falling_columns_end(oracle_tables, name):
    """Vs falling with depth: the Love phase curve ends at 20 s (on two knots at 12 s already), the Love group curve at 16 s, in
    every model down to 45 km; the depth kernels of those entries are 0.  Every other curve of every case is complete, the
    Rayleigh entries of the falling column included."""
    c = CASES[name]
    pv, sen = oracle_tables(name)
    off, K = T.offsets(c["segments"])
    ended = {(int(k), int(col)) for k, col in zip(*np.nonzero(pv == 0))}
    col = c["falling"]
    if name not in TC.FALLING_ENDS:
        assert col is None and ended == set()
        return
    lc = (off[1] + 1, off[1] + 2) if name == "two_knots" else (off[1] + 2,)
    assert ended == {(k, col) for k in lc} | {(off[2] + 1, col)}
    assert (pv[:off[1], col] != 0).all()
    if sen is not None:
        for q in range(3):
            assert all(not sen[q][:, k, cc].any() for k, cc in ended)
        assert (sen[0][:, :off[1], col] != 0).all()
