"""-m gpu: dazim_dispersion_kernels_typed (csrc/disp_typed.hip) where its host code splits the work and lays out the LDS in another
way than on the common model of tests/test_disp_typed_gpu.py -- the cases of tests/typed_cases.py, which tests/test_typed_cases_cpu.py
shows to give 32, 16 and 8 items per workgroup (idle lanes, a patch stride 3 tw, col0 and cpb that follow tw), 2 and 64 knots, a
patch that is the whole stack, one column, 60 periods, and partial last workgroups throughout.

Per case:
  exact    every table is bit-equal to depthkernel composed of dazim_surfdisp96 calls on host-built stacks (device against device,
           as tests/test_disp_typed_gpu.py does on the common model): the lane / variant / column bookkeeping at every tw;
  the path ran: stat disp_typed.items_per_wg after the call is what typed_cases.plan gives -- a change of the host's LDS formula
           cannot turn the fallback cases back into 64-item runs unnoticed, and the Python mirror cannot drift;
  oracle   typed_kernels_ref.check_tables against the oracle-driven yardstick (= the reference's, tests/test_typed_cases_cpu.py)
           under the bars of tests/test_surfdisp_full_gpu.py, none widened: the per-entry bars (C_ULP, U_ABS and their quotient
           form) case by case, the bit-equal shares on the entries of all cases pooled per wave type and table (several cases
           have a few dozen entries, where a 1 % allowance means nothing);
  ended    where the falling column's Love curves end: zeros in pv and in all three kernels, counted in n_failed.
Then the segment order (the Rayleigh-phase slice anywhere but first: koff != 0 in the 2-D copy of its kernels), scratch reuse
across shapes, and the refusals of the host (more than NL layers, nz outside 2 .. 64): argument checks, nothing runs.

Measured on an MI355X: every table of every case is bit-equal to the composed call and to the oracle (max |d| 0, every share 1.0,
the 190-, 197- and 117-layer stacks included), so no case needs the rough bars of tests/test_surfdisp_full_gpu.py; the items per
workgroup are the plan's (64, 64, 32, 16, 32, 16, 8, 64, 32, 64, 64 in the order of typed_cases.cases()).  The file takes 8 s, 3 s
of them the oracle's.

What a wrong kernel would trip here while tests/test_disp_typed_gpu.py (tw = 64, koff[irc] = 0) cannot notice, by the code:
  patch stride 3 TW for 3 tw     lanes read rows they did not write wherever tw < 64: the exact leg of patch_tw32 and patch_tw16;
  cpb without its + 1            a workgroup that holds the tail of one column and the head of the next has one table where it
                                 needs two: the exact leg of max_knots (the other cases' workgroups happen to span no more than
                                 ceil(tw / nvar) columns); and the smaller LDS sum keeps curves_tw32_first at 64 items: the
                                 items-per-workgroup test;
  no koff[irc] ncol in the copy  the Rayleigh-phase kernels land in rows 0 ..: test_segment_order, both orders;
  active without lane < tw       lanes tw .. 63 run the next workgroup's items on patch rows that lanes 0 .. tw - 1 overwrite, and
                                 store to the same cg entries as that workgroup: the exact leg of patch_tw32 / patch_tw16 fails
                                 unless every one of those doubled stores (32 x 3 and more) happens to land first."""
import numpy as np
import pytest

from tests import typed_cases as TC
from tests import typed_kernels_ref as T

pytestmark = pytest.mark.gpu
CASES = TC.cases()
QN = ("sen_vs", "sen_vp", "sen_rho")


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def run(ctx, c):
    """one call of the shared context -> (pv, sen, nf, items per workgroup the call reported)"""
    pv, sen, nf = ctx.dispersion_kernels_typed(c["vel"], c["depz"], c["segments"], c["sublayers"], kernels=c["kernels"])
    frozen(pv, *(sen or ()))
    return pv, sen, nf, int(ctx.stat("disp_typed.items_per_wg"))


def lazily(make):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = make(name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def got(ctx):
    """{name: (pv, sen, nf, items per workgroup)} of the device, each computed once and left alone"""
    return lazily(lambda name: run(ctx, CASES[name]))


@pytest.fixture(scope="module")
def composed(ctx):
    """{name: (pv, sen)} of depthkernel composed of dazim_surfdisp96 calls, one batched call per segment"""
    def make(name):
        pv, sen = TC.tables(CASES[name], ctx.surfdisp96, batched=True)
        frozen(pv, *(sen or ()))
        return pv, sen
    return lazily(make)


@pytest.fixture(scope="module")
def want(orc):
    """{name: (pv, sen)} of the oracle-driven yardstick"""
    def make(name):
        pv, sen = TC.tables(CASES[name], orc.surfdisp96_full)
        frozen(pv, *(sen or ()))
        return pv, sen
    return lazily(make)


@pytest.fixture(scope="module")
def common(ctx):
    """the four-segment call on the common model, (pv, sen, nf), and the same curves only"""
    vel = T.common_model()
    full = ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS, T.SUBLAYERS)
    curves = ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS, T.SUBLAYERS, kernels=False)
    frozen(vel, full[0], curves[0], *full[1])
    return vel, full, curves


def same_bits(what, x, y):
    """(pv, sen, nf, ...) twice; names the first entry that differs"""
    assert x[2] == y[2], (what, "n_failed", x[2], y[2])
    bad = np.argwhere(x[0] != y[0])
    assert len(bad) == 0, f"{what} pv: {len(bad)} entries differ, first (k, col) {bad[0]}"
    assert (x[1] is None) == (y[1] is None), what
    for q, (a, b) in enumerate(zip(x[1] or (), y[1] or ())):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what} {QN[q]}: {len(bad)} entries differ, first (knot, k, col) {bad[0]}"


# ---- 1, 2: the exact leg, and the plan that ran ----
@pytest.mark.parametrize("name", list(CASES))
def test_tables_equal_depthkernel_composed_of_surfdisp96(got, composed, name):
    c, p = CASES[name], TC.case_plan(CASES[name])
    pv, sen, nf, items = got(name)
    cpv, csen = composed(name)
    K = sum(len(t) for _, _, t in c["segments"])
    assert pv.shape == (K, p.ncol) and np.isfinite(pv).all() and all(np.isfinite(s).all() for s in sen or ())
    assert (sen is None) == (not c["kernels"])
    print(f"\n[{name}] items per workgroup {items} (plan {p.tw}), cpb {p.cpb}, lds {p.lds}, workgroups {p.blocks}, failed {nf}")
    same_bits(name, (pv, sen, nf), (cpv, csen, int((cpv == 0).sum())))
    if csen is not None:
        assert (csen[0] != 0).mean() > 0.5                # (the comparison is not one of zeros)


@pytest.mark.parametrize("name", list(CASES))
def test_the_planned_items_per_workgroup_ran(got, name):
    assert got(name)[3] == TC.case_plan(CASES[name]).tw


# ---- 3: the oracle leg ----
def test_every_case_against_the_cpu_oracle(got, want):
    """Per-entry bars case by case, bit-equal shares pooled over the cases per wave type and table (typed_kernels_ref.check_tables,
    check_pooled_shares).  max_knots, curves_tw16 and curves_tw8 are the first comparisons of dazim_surfdisp96's functions with
    the oracle on more than 40 layers (190, 117, 197)."""
    pool = {}
    for name, c in CASES.items():
        pv, sen, _, _ = got(name)
        T.check_tables(f"{name}: device vs oracle", (pv, sen), want(name), c["vel"], c["segments"], pool=pool)
    T.check_pooled_shares("all cases: device vs oracle", pool)


# ---- 4: ended curves under every split ----
@pytest.mark.parametrize("name", TC.FALLING_ENDS)
def test_ended_curves_are_zeros_and_a_count(got, want, name):
    c = CASES[name]
    pv, sen, nf, _ = got(name)
    wpv = want(name)[0]
    off, K = T.offsets(c["segments"])
    col = c["falling"]
    ended = np.argwhere(wpv == 0)
    assert len(ended) >= 2 and (ended[:, 1] == col).all() and (ended[:, 0] >= off[1]).all()     # Love entries of the falling column
    assert np.array_equal(pv == 0, wpv == 0) and nf == len(ended)
    assert (pv[:off[1], col] != 0).all()                                                        # its Rayleigh curve is complete
    if sen is not None:
        for k, cc in ended:
            assert all(not s[:, k, cc].any() for s in sen), (name, k, cc)
        assert (sen[0][:, :off[1], col] != 0).all()


# ---- 5: segment order ----
@pytest.mark.parametrize("order", [(3, 0, 1, 2), (2, 0)], ids=["Lg-Rc-Rg-Lc", "Lc-Rc"])
def test_segment_order(ctx, common, order):
    """the Rayleigh-phase segment second: its curves land at koff x ncol, its depth kernels through the 2-D copy with a row offset"""
    vel, full, curves = common
    off, K = T.offsets(T.SEGMENTS)
    segs = [T.SEGMENTS[s] for s in order]
    rows = np.concatenate([np.arange(off[s], off[s] + len(T.SEGMENTS[s][2])) for s in order])
    for ref, kernels in ((full, True), (curves, False)):
        pv, sen, nf = ctx.dispersion_kernels_typed(vel, T.DEPZ, segs, T.SUBLAYERS, kernels=kernels)
        assert int(ctx.stat("disp_typed.items_per_wg")) == 64
        wsen = [s[:, rows] for s in ref[1]] if kernels else None
        same_bits(f"order {order}, kernels={kernels}", (pv, sen, nf), (ref[0][rows], wsen, int((ref[0][rows] == 0).sum())))
    assert (full[1][0][:, off[0]:off[1]] != 0).all()      # (the Rayleigh-phase kernels are not zeros)


# ---- 6: scratch reuse ----
def test_scratch_reuse_across_shapes(ctx, common, got):
    """20 columns x 31 / 21 variants on 17 layers, then 16 items per workgroup on 152 layers, then 64 knots, then the first again:
    dispt.cg and the other named scratch buffers serve all of them"""
    vel, full, _ = common
    same_bits("the common model", ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS, T.SUBLAYERS), full)
    for name in ("patch_tw16", "max_knots"):
        again = run(ctx, CASES[name])
        same_bits(f"{name} again", again, got(name))
        assert again[3] == got(name)[3]
    same_bits("the common model after them", ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS, T.SUBLAYERS), full)


# ---- 7: refusals ----
def test_refused_shapes_leave_the_context_usable(ctx, common):
    """253 layers (64 knots at sublayers 3) exceed NL; 65 knots and 1 knot are outside 2 .. NZMAX.  The host refuses all three
    before anything is launched, and the next call gives the common model's tables."""
    vel, full, _ = common
    one = lambda nz: np.full((nz, 1, 1), 3.5, np.float32)
    refused = [(2.0 * np.arange(64), 3.0, "NL"), (2.0 * np.arange(65), 1.0, "nz"), (np.zeros(1), 3.0, "nz")]
    for depz, sublayers, word in refused:
        with pytest.raises(RuntimeError, match=word):
            ctx.dispersion_kernels_typed(one(len(depz)), depz, TC.SEGMENTS, sublayers)
        same_bits(f"the common model after {len(depz)} knots", ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS, T.SUBLAYERS), full)
