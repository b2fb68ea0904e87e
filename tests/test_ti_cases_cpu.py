"""CPU (-m "not gpu"): the stress inputs of tests/ti_cases.py do take the TI path through the saturation branches of tregn96, the
oracle (oracle/tregn.c) agrees with the compiled reference on them (tests/golden/ti_stress.npz, written by
tests/golden/make_ti_stress_golden.py), and the inputs of tests/test_ti_gpu.py take none of those branches -- which is why
tests/test_ti_edges_gpu.py exists.

Branch census (oracle.pyoracle.Oracle.ti_census) per run, counts of the six stress runs A/B x minthk 0.5, 1, 3 (1 176, 2 352 and
4 704 finite-layer visits):
    fac0 758-1176   dfac0 344-538   ffunc 168-504   gfunc 0-261 (A at minthk 3: 0, B at minthk 3: 16)   h1func 315-504
    h2func 168-504   ext80 168-633   flush 313-1239   imag_rsv 185-771   imag_rp 0-21 (B at minthk 1 and 3 only)
and of the four inputs of tests/test_ti_gpu.py (58 752, 97 920, 93 636 and 1 536 visits): 0 on all eight saturation branches,
imag_rsv 501-25 192.

Not reached by any input here, the single very thick deep layer of ti_cases.thick_deep_layer (a 360 km layer at T = 1 s and 2 s)
included: the `down` cut-off |pex - svex| > 40 (down0), the two t1 < 1e-40 resets (t1_up, t1_down) and the tiny-nu special cases
(tiny_nu).  They need a layer whose P and SV exponents differ by 40 without either wave having decayed to nothing above it, a
vector that underflows in one layer, or a phase velocity equal to a layer velocity to 1e-8: no Earth column does that."""
import os

import numpy as np
import pytest

from tests import ti_cases as K

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ti_stress.npz")


@pytest.fixture(scope="module")
def runs(orc):
    """{key: (pv, lsen, census)} of the oracle on the six stress runs"""
    out = {}
    orc.ti_census()
    for key, name, minthk in K.stress_runs():
        pv, ls = orc.depthkernel_ti(K.stress(name), K.DEPZ, K.T, minthk)
        out[key] = (pv, ls, orc.ti_census())
    return out


def test_oracle_against_reference(runs):
    """identical phase velocities and exact-zero pattern; per lane within the TI bar; per entry within R_CPU, which this test
    measures (it prints the figure)"""
    gold = np.load(GOLD)
    worst = 0.0
    for key, (pv, ls, _) in runs.items():
        pv_r, ls_r = gold[f"{key}_pv"], gold[f"{key}_lsen"]
        assert ls.shape == (7, 8, 21) and np.isfinite(ls).all() and (pv > 0).all(), key
        assert np.array_equal(pv, pv_r), key
        assert np.array_equal(ls == 0, ls_r == 0), key
        assert 160 <= int((ls_r == 0).sum()) <= 200, key            # (the zeros are the deep layers of the short periods, not a dead run)
        lane = K.lane_excess(ls, ls_r)
        rel, at = K.entry_excess(ls, ls_r, floor=0.0)   # every non-zero entry
        print(f"{key}: per lane {lane:.3g}, per entry {rel:.3g} at {at}, smallest non-zero |Lsen| {np.abs(ls_r[ls_r != 0]).min():.3g}")
        assert lane <= K.LANE_TOL, (key, lane)
        worst = max(worst, rel)
    print(f"R_cpu = {worst:.3g}")
    assert worst <= K.R_CPU, worst


def test_measures_see_what_the_global_norm_hides():
    """a deep entry wrong by a factor 2, a lane wrong by 1e-5 of its own maximum and a non-zero where the reference has an exact zero
    all pass `max|diff| <= 1e-6 max|want|`; each is caught by its measure"""
    want = np.zeros((3, 2, 2), np.float32)
    want[:, 0, 0] = [1.0, 1e-3, 1e-20]
    want[:, 1, 1] = [1e-4, 1e-6, 0.0]
    deep, lane, zero = want.copy(), want.copy(), want.copy()
    deep[2, 0, 0] *= 2
    lane[0, 1, 1] += 1e-9
    zero[2, 1, 1] = 1e-12
    for got, lane_bad, entry_bad, zero_bad in ((deep, False, True, False), (lane, True, True, False), (zero, False, False, True)):
        got = got.astype(np.float32)
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
        assert (K.lane_excess(got, want) > K.LANE_TOL) == lane_bad
        assert (K.entry_excess(got, want)[0] > K.ENTRY_TOL_GPU) == entry_bad
        assert (K.small_ceiling(got, want) >= K.ZERO_CEIL) == zero_bad
    assert K.entry_excess(want, want, floor=0.0) == (0.0, (0, 0, 0)) and K.lane_excess(want, want) == 0.0


def test_stress_runs_take_every_listed_branch(runs):
    total = {k: sum(c[k] for _, _, c in runs.values()) for k in K.MUST_REACH + K.NOT_REACHED + ("layers",)}
    print(total)
    assert [c["layers"] for _, _, c in runs.values()] == [1176, 2352, 4704] * 2     # 168 lanes x 7, 14, 28 finite layers
    for k in K.MUST_REACH:
        assert total[k] >= 1, (k, total)
    # the thin ones, and the runs that carry them
    assert runs["A_0.5"][2]["gfunc"] >= 1 and runs["B_3"][2]["gfunc"] >= 1
    assert runs["B_3"][2]["imag_rp"] >= 1
    # every run on its own takes the branches push_up and the eigenfunction window depend on
    for key, (_, _, c) in runs.items():
        for k in ("fac0", "dfac0", "ext80", "flush", "imag_rsv"):
            assert c[k] >= 1, (key, k)


def test_thick_deep_layer_reaches_no_further_branch(orc, runs):
    """the one attempt at the branches of NOT_REACHED (module docstring): they stay at zero there and in the stress runs"""
    c = K.thick_deep_layer()
    orc.ti_census()
    pv, ls = orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    census = orc.ti_census()
    assert (pv > 0).all() and np.isfinite(ls).all()
    assert census["layers"] == 8 and census["dfac0"] >= 1 and census["gfunc"] >= 1
    for k in K.NOT_REACHED:
        assert census[k] == 0 and all(r[2][k] == 0 for r in runs.values()), k


def test_old_inputs_take_no_saturation_branch(orc):
    """negative control: the inputs of tests/test_ti_gpu.py (test4 columns at minthk 2 and 4, the test1 model, the random 5-knot
    model) take none of the eight saturation branches; an imaginary nu_sv is the only non-trivial path they reach"""
    orc.ti_census()
    visits = []
    for vel, depz, t, minthk in K.old_inputs():
        orc.depthkernel_ti(vel, depz, t, minthk)
        c = orc.ti_census()
        visits.append(c["layers"])
        for k in K.SATURATION + ("imag_rp",) + K.NOT_REACHED:
            assert c[k] == 0, (k, c)
        assert c["imag_rsv"] > 0
    assert visits == [58752, 97920, 93636, 1536]


def test_census_changes_no_number_and_resets(orc):
    """counting is counting only: two runs give the same bits whatever the counters hold, read without reset keeps them"""
    vel = K.stress("B")
    orc.ti_census()
    a = orc.depthkernel_ti(vel, K.DEPZ, K.T, 3.0)
    first = orc.ti_census(reset=False)
    assert first == orc.ti_census(reset=False) and first["layers"] == 4704
    b = orc.depthkernel_ti(vel, K.DEPZ, K.T, 3.0)
    second = orc.ti_census()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(second[k] == 2 * first[k] for k in first)
    assert not any(orc.ti_census().values())


def test_oracle_refuses_models_beyond_its_arrays(orc):
    """an 8-knot model at minthk 80 refines to 568 layers > NL = 200, 61 periods > NP = 60: an error, not a write past the arrays"""
    vel = K.stress("A")
    with pytest.raises(RuntimeError, match="rc=-4"):
        orc.depthkernel_ti(vel, K.DEPZ, K.T, 80.0)
    with pytest.raises(RuntimeError, match="rc=-4"):
        orc.depthkernel(vel, K.DEPZ, K.T, 80.0)
    t61 = np.linspace(5.0, 35.0, 61)
    with pytest.raises(RuntimeError, match="rc=-4"):
        orc.depthkernel_ti(vel[:, :1, :1], K.DEPZ, t61, 1.0)
    with pytest.raises(RuntimeError, match="rc=-4"):
        orc.depthkernel(vel[:, :1, :1], K.DEPZ, t61, 1.0, kernels=False)
    c = K.layer_limit(201)
    with pytest.raises(RuntimeError, match="rc=-4"):
        orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    c = K.layer_limit(200)                                   # NL itself fits
    pv, ls = orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    assert (pv > 0).all() and np.isfinite(ls).all() and np.abs(ls).max() > 0
    c = K.fluid_column()
    with pytest.raises(RuntimeError, match="rc=3"):
        orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
