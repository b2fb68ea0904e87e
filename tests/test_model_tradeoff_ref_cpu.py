"""CPU: the NumPy statement of dazim_model_tradeoff (tests/model_tradeoff_ref.py) against what it must satisfy whatever computes it --
the closed-form evidence against the brute-force one, the monotone sides of the L-curve, tr(Rm) of model_posterior_ref -- and the
condition of every sweep point the GPU tests run on (cond(A_k) <= 1e4, and cond(P_k) <= 1e4 where P_k is positive definite: the fp64
factorisation error stays far below the GPU bar, which then measures the kernels and not the problems)."""
import functools

import numpy as np
import pytest

from tests import model_posterior_ref as mref
from tests import model_tradeoff_ref as ref

CASES = [(s, False) for s in mref.SHAPES_ISO] + [(s, True) for s in mref.SHAPES_JOINT]
CASE_IDS = [f"{'joint' if jt else 'iso'}-{nx}x{ny}x{nz}" for (nx, ny, nz), jt in CASES]
NCOMMON = len(ref.SCALES)


@functools.lru_cache(maxsize=None)
def solved(shape, joint, reg):
    prob = ref.problem(shape, joint, reg)
    scale, damp = ref.sweep(prob)
    return prob, scale, damp, ref.linalg(prob, scale, damp)


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_condition_of_the_gpu_sweeps(case, reg):
    """a condition, not a measurement; GCV's denominator stays away from 0 as well"""
    prob, scale, damp, out = solved(case[0], case[1], reg)
    D, L = mref.parts(prob)
    blk = ref.blocks(prob, L)
    assert not out["n_failed"].any()
    for k in range(len(damp)):
        P = ref.prior(prob, L, blk, scale[k], damp[k])
        assert np.linalg.cond(D + P) <= ref.COND_MAX
        assert ref.is_pd(P) and np.linalg.cond(P) <= ref.COND_MAX
    assert ((prob["m_data"] - out["dof"].sum(axis=1)) / prob["m_data"] >= 0.1).all()


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_closed_form_evidence_is_the_marginal_likelihood(case, reg):
    prob, scale, damp, out = solved(case[0], case[1], reg)
    for k in range(len(damp)):
        want = ref.brute_evidence(prob, scale[k], damp[k])
        assert abs(out["logev"][k] - want) <= 1e-9 * max(1.0, abs(want)), (k, out["logev"][k], want)


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_two_sides_of_the_l_curve_are_monotone(case, reg):
    """one common factor ascending at a fixed damping: |L x|^2 does not increase, chi2 + damp^2 |x|^2 does not decrease"""
    prob, scale, damp, out = solved(case[0], case[1], reg)
    per = len(damp) // len(ref.DAMP_FACTORS)
    for f in range(len(ref.DAMP_FACTORS)):
        sl = slice(f * per, f * per + NCOMMON)
        assert (scale[sl, 0] == np.float32(ref.SCALES)).all() and len(set(damp[sl])) == 1
        reg2 = out["reg2"][sl].sum(axis=1)
        misfit = out["chi2"][sl] + float(damp[sl][0]) ** 2 * out["xnorm2"][sl]
        assert (np.diff(reg2) <= 1e-10 * max(1.0, reg2.max())).all()
        assert (np.diff(misfit) >= -1e-10 * misfit.max()).all()


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dof_is_the_trace_of_the_resolution_matrix(case, reg):
    """at scale 1 and damping factor 1 the problem is model_posterior_ref's own: sum_b dof = tr(Rm)"""
    prob, scale, damp, out = solved(case[0], case[1], reg)
    k = [i for i in range(len(damp)) if (scale[i] == 1).all() and damp[i] == np.float32(prob["damp"])][0]
    want = mref.linalg(prob)["trace"].sum()
    assert abs(out["dof"][k].sum() - want) <= 1e-10 * max(1.0, want)


def test_a_singular_point_is_nan_alone():
    """no regularisation rows and damp 0: the cell no ray crosses leaves A_k singular at that point only"""
    prob = ref.problem((9, 5, 3), True, (0.0, 0.5))
    scale, damp = np.ones((3, 3), np.float32), np.array([0.5, 0.0, 0.3], np.float32)
    out = ref.linalg(prob, scale, damp)
    assert list(out["n_failed"]) == [0, 1, 0]
    for k in ref.OUTPUTS:
        assert np.isnan(out[k][1]).all() and np.isfinite(out[k][[0, 2]]).all(), k


def test_the_librarys_pick_is_the_numpy_statement():
    """dazim_tradeoff_pick is host code: the built library's function against `pick`, without a GPU"""
    import dazimsurftomo_amd as dz
    dz.build()
    ref.check_pick(dz.tradeoff_pick)


def test_pick_rules():
    chi2 = np.array([1.0, 1.1, 1.3, 4.0, 20.0])
    reg = np.array([50.0, 10.0, 1.0, 0.8, 0.7])
    got = ref.pick(chi2, reg, np.array([3.0, np.nan, 1.0, 1.0, 2.0]), np.array([-5.0, -2.0, np.inf, -2.0, -9.0]))
    assert got == dict(corner=2, gcv=2, evidence=1)
    assert ref.pick(chi2[:2], reg[:2], None, None) == dict(corner=-1, gcv=-1, evidence=-1)
    nan = np.full(5, np.nan)
    assert ref.pick(nan, reg, nan, nan) == dict(corner=-1, gcv=-1, evidence=-1)
