"""CPU: the yardstick of dazim_dispersion_kernels_typed (tests/typed_kernels_ref.py: depthkernel for one (iwave, igr) composed of
Brocher, refineGrid2LayerMdl and a surfdisp96 passed in) is the reference's.  Driven by the oracle's surfdisp96 it is compared with
itself driven by the reference subroutine, on the common model, for all four wave types, under the bars that
tests/test_disp_typed_gpu.py holds the device to (typed_kernels_ref.check_tables) -- so those caps hold for the reference alone --
and, for Rayleigh phase, with the reference's own depthkernel.  Skipped where the reference has not been compiled (oracle/_ref).
It passes before dazim_dispersion_kernels_typed exists: that is its job."""
import numpy as np
import pytest

from oracle.pyoracle import Ref
from tests import typed_kernels_ref as T
from tests.bars import within

needs_ref = pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libdazim_ref.so not built")


@pytest.fixture(scope="module")
def vel():
    return T.common_model()


@pytest.fixture(scope="module")
def oracle_tables(orc, vel):
    return T.typed_tables(vel, T.DEPZ, T.SUBLAYERS, T.SEGMENTS, orc.surfdisp96_full)


@needs_ref
def test_oracle_driven_yardstick_against_the_reference_driven_one(oracle_tables, vel):
    want = T.typed_tables(vel, T.DEPZ, T.SUBLAYERS, T.SEGMENTS, Ref().surfdisp96_full)
    T.check_tables("oracle vs reference", oracle_tables, want, vel, T.SEGMENTS)


@needs_ref
def test_rayleigh_phase_yardstick_is_the_references_depthkernel(vel):
    """the composition itself (perturbation order, fp32 roundings, denominator): bit for bit the reference's depthkernel"""
    iw, ig, t = T.SEGMENTS[0]
    pv, sen = T.depthkernel_typed(vel, T.DEPZ, T.SUBLAYERS, iw, ig, t, Ref().surfdisp96_full)
    pvr, senr = Ref().depthkernel(vel, T.DEPZ, t, T.SUBLAYERS)
    assert (pv != 0).all() and np.array_equal(pv, pvr)
    for a, b in zip(sen, senr):
        assert np.array_equal(a, b)


def test_rayleigh_phase_yardstick_is_the_oracles_depthkernel(orc, oracle_tables, vel):
    pvo, seno = orc.depthkernel(vel, T.DEPZ, T.SEGMENTS[0][2], T.SUBLAYERS)
    k = len(T.SEGMENTS[0][2])
    assert np.array_equal(oracle_tables[0][:k], pvo)
    for a, b in zip(oracle_tables[1], seno):
        assert np.array_equal(a[:, :k], b)


def test_where_the_love_curves_of_the_special_columns_end(oracle_tables):
    """the failure cases the device tests rely on are in the model: no root from a period on = zeros from there on"""
    pv = oracle_tables[0]
    off, K = T.offsets(T.SEGMENTS)
    ended = {(int(k), int(c)) for k, c in zip(*np.nonzero(pv == 0))}
    assert ended == {(off[2] + 2, T.COL_UNIFORM), (off[2] + 2, T.COL_FALLING), (off[3] + 1, T.COL_FALLING)}
    for q in range(3):
        for k, c in ended:
            assert not oracle_tables[1][q][:, k, c].any()
    assert (pv[:off[2]] != 0).all()                       # every Rayleigh entry has a root


def test_the_references_love_vp_kernel_is_search_noise(orc, vel):
    """What dazim_dispersion_kernels_typed defines as 0: the two Vp copies of a Love segment are the same layers for the SH period
    equation and differ in the start value of the first search only.  Each search stops within nevill's tolerance 1e-6 c of the
    root (inv/surfdisp96.f:608) and is rounded to fp32, so two curves differ by at most 2e-6 c + one fp32 ulp of c (C_ULP) -- times
    1 / (2 h) = 100 for a group velocity, the quotient of two such roots h = 0.5 % apart in period."""
    from tests.test_surfdisp_full_gpu import C_ULP
    base = T.brocher_knots(vel)
    for iw, ig, t in T.SEGMENTS[2:]:
        pv, sen = T.depthkernel_typed(vel, T.DEPZ, T.SUBLAYERS, iw, ig, t, orc.surfdisp96_full, love_vp_zero=False)
        dcg = np.abs(sen[1]) * (np.float64(0.01) * base[1].astype(np.float64))[:, None, :]        # |cg2 - cg1|
        tol = (2e-6 * pv.max() + C_ULP) * (100.0 if ig else 1.0)
        print(f"\n[love vp] igr={ig}: non-zero entries {(sen[1] != 0).sum()} of {sen[1].size}, max |sen_vp| {np.abs(sen[1]).max():.2e}, "
              f"max |sen_vs| {np.abs(sen[0]).max():.2e}")
        within(f"Love igr={ig} |cg2 - cg1| of the Vp copies, km/s", dcg.max(), tol)
        pz, sz = T.depthkernel_typed(vel, T.DEPZ, T.SUBLAYERS, iw, ig, t, orc.surfdisp96_full)
        assert not sz[1].any() and np.array_equal(pz, pv) and np.array_equal(sz[0], sen[0]) and np.array_equal(sz[2], sen[2])
