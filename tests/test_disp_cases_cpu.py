"""CPU (-m "not gpu"): the inputs of tests/disp_cases.py do take the dispersion path through the guards of surfdisp96's secular
function and the turns of its root search, the oracle (oracle/disp.c) equals the compiled reference on them BIT FOR BIT
(tests/golden/disp_stress.npz, written by tests/golden/make_disp_stress_golden.py), and the inputs of tests/test_disp_gpu.py take
none of the saturation branches -- which is why tests/test_disp_edges_gpu.py exists.

Branch census (oracle.pyoracle.Oracle.disp_census), counts per run with depth kernels (49 variants per column):
    the six stress runs (3.3 M - 16.9 M layer visits): p_sat 1.0 M - 3.5 M (14-35 % of the visits), s_sat 0.9 M - 3.2 M, a0_zero
        0.7 M - 1.9 M, p_osc 29 k and 99 k (B at minthk 1 and 3 only), getsol_down 402 - 1 365 (B only)
    0.2 .. 1 s: 2.8 M - 3.0 M visits, p_sat 73-81 %, s_sat 70-78 %, a0_zero 59-66 %
    B decreasing: getsol_down 5 557 of 8 232 searches; B shuffled: nev_c3_out 227, nev_denom 1
    1e5 s and 1e6 s appended: omega_clamp 206 k / 290 k evaluations, exit_window 1 029 (21 columns x 49 variants, whose second
        failing period is never searched), 42 of 126 phase velocities 0
    B at minthk 3, 80 s first: first_over_512 1 029, the longest walk 582 steps (580 among the columns' own curves)
and of the eight oracle runs behind tests/test_disp_gpu.py (135 M visits): 0 on p_sat, s_sat, a0_zero, p_osc and omega_clamp.

Not reached by any input here, the attempts of disp_cases.attempts() included: wvno == xka or xkb to the last bit (p_equal, s_equal),
a compound vector below 1e-40 (t1_tiny: it is rescaled after every layer and a0 is cut to 0 long before), Neville's m > 10 and
its 100-pass limit (nev_m_cap, nev_nctrl: the 1e-6 c bracket is reached in fewer than 20 passes), and of the search c2 <= clow
(getsol_turn), c1 < cm (exit_below_cm) and a refined root above betmx (exit_root_above): a downward walk always meets the sign
change above the start value, which lies below every root, and the window closes at betmx + dc before a root above betmx."""
import numpy as np
import pytest

from tests import disp_cases as D


@pytest.fixture(scope="module")
def runs(orc):
    """{name: (pv, sen, census)} of the oracle on every case, computed once and left alone"""
    out = {}
    orc.disp_census()
    for name, c in D.cases().items():
        pv, sen = orc.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"], kernels=c["kernels"])
        out[name] = (pv, sen, orc.disp_census())
    return out


def test_oracle_equals_the_compiled_reference_bit_for_bit(runs):
    """DESIGN.md section 2's pin, where the guards switch: phase velocities and the three tables, every bit"""
    gold = np.load(D.GOLD)
    assert sorted(gold.files) == sorted(f"{k}_{a}" for k in D.GOLDEN_KEYS for a in ("pv", "sen_vs", "sen_vp", "sen_rho"))
    for key in D.GOLDEN_KEYS:
        pv, sen, _ = runs[key]
        assert pv.shape == (8, 21) and (pv > 0).all(), key
        assert np.array_equal(pv, gold[f"{key}_pv"]), key
        for name, s in zip(("vs", "vp", "rho"), sen):
            ref = gold[f"{key}_sen_{name}"]
            assert s.shape == (8, 8, 21) and np.isfinite(s).all()
            assert np.array_equal(s, ref), (key, name, np.abs(s - ref).max())
            zeros = float((ref == 0).mean())
            print(f"{key} sen_{name}: exact zeros {zeros:.3f}")
            # the knots the wave no longer reaches: a third of the entries on the stress runs, two thirds at 0.2 .. 1 s
            assert (0.33 <= zeros <= 0.44) if key in D.STRESS_KEYS else (0.66 <= zeros <= 0.76), (key, name, zeros)


def test_new_inputs_take_every_listed_branch(runs):
    for k in D.MUST_REACH:
        c = runs[D.REACHED_BY[k]][2]
        print(k, D.REACHED_BY[k], c[k], "of", c["layers"], "visits")
        assert c[k] >= 1, (k, D.REACHED_BY[k], c)
    # every stress run and both short runs saturate on their own, in all three guards; the short ones in most of their visits
    for key in D.GOLDEN_KEYS + ("B_2",):
        c = runs[key][2]
        for k in D.SATURATION:
            assert c[k] >= 0.05 * c["layers"], (key, k, c)
    for key in ("A_1_short", "B_1_short"):
        c = runs[key][2]
        assert c["p_sat"] >= 0.7 * c["layers"] and c["s_sat"] >= 0.7 * c["layers"] and c["a0_zero"] >= 0.55 * c["layers"], c
    assert [runs[k][2]["layers"] for k in D.STRESS_KEYS] == [3384479, 7071316, 14467796, 3348968, 7845936, 16873248]
    assert runs["B_1"][2]["p_osc"] >= 1 and runs["B_2"][2]["p_osc"] >= 1
    assert runs["B_1_decreasing"][2]["getsol_down"] > runs["B_1"][2]["getsol_down"]
    # failures: both appended periods of every column, through betmx + dc; the first period of the narrow columns; mid-curve
    for key in ("A_1_long", "B_1_long"):
        pv, _, c = runs[key]
        assert (pv[:4] > 0).all() and (pv[4:] == 0).all() and pv.size == 126
        assert c["omega_clamp"] > 0 and c["exit_window"] == 21 * 49 and c["exit_below_cm"] == c["exit_root_above"] == 0
    pv, sen, c = runs["first_fails"]
    assert (pv == 0).all() and all((s == 0).all() for s in sen) and c["exit_window"] == c["getsol"] == 3 * 25
    pv, _, c = runs["A_1_80first"]
    assert (pv[0] > 0).all() and int((pv == 0).sum()) == 8 and c["exit_window"] > 0


def test_planted_block_edges_and_long_walks(orc, runs):
    """the columns' own curves (no depth kernels, which is what disp_bracket_kernel sees): the first period's walk ends at exactly
    the grid point disp_cases.py says"""
    cases = D.cases()

    def own(c, cols=None):
        vel = c["vel"] if cols is None else np.ascontiguousarray(c["vel"][:, :, cols])
        orc.disp_census()
        pv, _ = orc.depthkernel(vel, c["depz"], c["t"], c["minthk"], kernels=False)
        return pv, orc.disp_census()

    for t1, steps in D.PLANTED:
        c = cases[f"planted_{steps}"]
        assert c["t"][0] == t1 and c["vel"].shape == (8, 1, 1)
        pv, cen = own(c)
        assert cen["first_steps_max"] == steps and (pv > 0).all(), (steps, cen)
        assert cen["first_over_512"] == (1 if steps > D.FF_POINTS else 0)
    # the in-block cut: column 0 walks 251 = 3 * 64 + 59 steps to betmx + dc, the others 202 and 235; all three fail at once
    walked = []
    for i in range(3):
        pv, cen = own(cases["first_fails"], slice(i, i + 1))
        assert (pv == 0).all() and cen["exit_window"] == 1 and cen["getsol"] == 1
        walked.append(cen["first_steps_max"])
    assert walked == [251, 202, 235] and all(w % 64 not in (0, 63) for w in walked)
    # the walk past the 512 points of disp_bracket_kernel: every one of the 21 columns, the longest 580 steps
    pv, cen = own(cases["B_3_80first"])
    print("B at minthk 3, 80 s first: columns beyond 512 steps", cen["first_over_512"], "longest", cen["first_steps_max"])
    assert cen["first_over_512"] == 21 and cen["first_steps_max"] == 580 and (pv > 0).all()
    assert runs["B_3_80first"][2]["first_steps_max"] == 582 and runs["B_3_80first"][2]["first_over_512"] == 21 * 49
    assert D.FOUND_BY_BRACKET_KERNEL == tuple(s for _, s in D.PLANTED if s + 1 < D.FF_POINTS)
    pv, cen = own(cases["A_1_80first"])
    assert cen["first_over_512"] == 0 and 256 < cen["first_steps_max"] < 512


def test_not_reached_stays_not_reached(orc, runs):
    """the list stays true: no case and no attempt of disp_cases.attempts() takes a branch of NOT_REACHED"""
    for name, (_, _, c) in runs.items():
        for k in D.NOT_REACHED:
            assert c[k] == 0, (name, k)
    orc.disp_census()
    for i, c in enumerate(D.attempts()):
        pv, _ = orc.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"], kernels=c["kernels"])
        cen = orc.disp_census()
        assert np.isfinite(pv).all() and cen["layers"] > 0
        for k in D.NOT_REACHED:
            assert cen[k] == 0, (i, k, cen)
    assert set(D.MUST_REACH).isdisjoint(D.NOT_REACHED)


def test_old_inputs_take_no_saturation_branch(orc):
    """negative control: the oracle runs behind tests/test_disp_gpu.py take none of the three saturation guards, no oscillatory P
    part and no omega clamp; oscillatory S, bisection restarts and (LVZ, rough columns) downward starts are all they reach"""
    orc.disp_census()
    visits = 0
    for c in D.old_inputs():
        orc.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"], kernels=c["kernels"])
        cen = orc.disp_census()
        visits += cen["layers"]
        for k in D.SATURATION + ("p_osc", "omega_clamp", "first_over_512") + D.NOT_REACHED:
            assert cen[k] == 0, (k, cen)
        assert cen["s_osc"] > 0 and cen["first_steps_max"] <= 302
    print("layer visits of the old inputs:", visits)
    assert visits > 100e6


def test_census_changes_no_number_and_resets(orc):
    """counting is counting only: two runs give the same bits whatever the counters hold, read without reset keeps them, the
    longest walk is a maximum and not a sum"""
    c = D.cases()["planted_128"]
    orc.disp_census()
    a = orc.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"])
    first = orc.disp_census(reset=False)
    assert first == orc.disp_census(reset=False) and first["getsol"] == 49 * 4
    b = orc.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"])
    second = orc.disp_census()
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert all(second[k] == 2 * first[k] for k in first if k != "first_steps_max")
    assert second["first_steps_max"] == first["first_steps_max"] == 129
    assert not any(orc.disp_census().values())
