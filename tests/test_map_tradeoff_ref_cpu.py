"""CPU: the NumPy statement of dazim_map_tradeoff (tests/map_tradeoff_ref.py) against what it must satisfy whatever computes it -- the
closed-form evidence per period against the brute-force one, the evidence of the whole block-diagonal system against the sum over the
periods, the library's host-only total and pick -- and the conditions of every (period, point) the GPU tests run on: cond(A) <= 1e4,
cond(P) <= 1e4 where P is positive definite, and (m_p - sum dof)/m_p >= 0.05, so that the fp64 factorisation error and GCV's
denominator stay far from the GPU bar, which then measures the kernels and not the problems.
Measured over the 3 024 (period, point)s: largest cond(A) 4.7e2, largest cond(P) 1.8e3, smallest (m_p - dof)/m_p 0.078, smallest m_p 5."""
import functools

import numpy as np
import pytest

from tests import map_posterior_ref as mref
from tests import map_tradeoff_ref as ref
from tests import model_tradeoff_ref as tref

CASES = [(s, False) for s in mref.SHAPES_ISO] + [(s, True) for s in mref.SHAPES_JOINT]
CASE_IDS = [f"{'azim' if az else 'iso'}-{nx}x{ny}" for (nx, ny), az in CASES]


@functools.lru_cache(maxsize=None)
def solved(shape, azim, reg, kmax):
    prob = ref.problem(shape[0], shape[1], kmax, azim, reg)
    scale, damp = ref.sweep(prob)
    return prob, scale, damp, ref.linalg(prob, scale, damp)


@pytest.mark.parametrize("kmax", [1, 3])
@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_condition_of_the_gpu_sweeps(case, reg, kmax):
    """conditions, not measurements (the figures are printed)"""
    prob, scale, damp, out = solved(case[0], case[1], reg, kmax)
    nblk = 3 if case[1] else 1
    assert not out["n_failed"].any()
    ca = cp = 0.0
    for part in ref.periods(prob):
        D = part["G"].T @ part["G"]
        for k in range(len(damp)):
            P = ref.prior(part, nblk, scale[k], damp[k])
            ca = max(ca, np.linalg.cond(D + P))
            if ref.is_pd(P):
                cp = max(cp, np.linalg.cond(P))
    slack = ((out["mdata_p"][None, :] - out["dof"].sum(axis=2)) / out["mdata_p"][None, :]).min()
    print(f"\n[measured] cond(A) {ca:.2e} cond(P) {cp:.2e} (m_p - dof)/m_p {slack:.3f} m_p {out['mdata_p'].min()}")
    assert ca <= ref.COND_MAX and cp <= ref.COND_MAX
    assert slack >= 0.05


@pytest.mark.parametrize("reg", mref.REGS, ids=mref.REG_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_closed_form_evidence_is_the_marginal_likelihood(case, reg):
    """per period against log N(b_p; 0, I + G_p P^-1 G_p^T), and the sum over the periods against the same expression for the whole
    matrix at once (the periods' G and P as the diagonal blocks of one system)"""
    prob, scale, damp, out = solved(case[0], case[1], reg, 3)
    nblk = 3 if case[1] else 1
    parts = ref.periods(prob)
    ng = parts[0]["G"].shape[1]
    tot = ref.totals(out)
    for k in range(len(damp)):
        Ps = [ref.prior(part, nblk, scale[k], damp[k]) for part in parts]
        for p, part in enumerate(parts):
            want = ref.brute_evidence(part["G"], part["b"], Ps[p])
            assert abs(out["logev"][k, p] - want) <= 1e-9 * max(1.0, abs(want)), (k, p, out["logev"][k, p], want)
        mp = [len(part["b"]) for part in parts]
        G, P = np.zeros((sum(mp), 3 * ng)), np.zeros((3 * ng, 3 * ng))
        for p, part in enumerate(parts):
            G[sum(mp[:p]):sum(mp[:p + 1]), p * ng:(p + 1) * ng] = part["G"]
            P[p * ng:(p + 1) * ng, p * ng:(p + 1) * ng] = Ps[p]
        want = ref.brute_evidence(G, np.concatenate([part["b"] for part in parts]), P)
        assert abs(tot["logev"][k] - want) <= 1e-9 * max(1.0, abs(want)), (k, tot["logev"][k], want)


def test_a_period_without_data_follows_the_formulas():
    prob = ref.without_data(ref.problem(9, 5, 3, True, mref.REGS[0]), 1)
    scale, damp = ref.sweep(prob)
    out = ref.linalg(prob, scale, damp)
    assert out["mdata_p"][1] == 0 and not out["n_failed"].any()
    x = out["x"].reshape(len(damp), 3, 3, -1)
    assert (x[:, :, 1] == 0).all() and (out["chi2"][:, 1] == 0).all() and (out["dof"][:, 1] == 0).all()
    assert np.isnan(out["gcv"][:, 1]).all() and np.isfinite(out["logev"]).all() and np.isfinite(out["gcv"][:, [0, 2]]).all()


def test_the_librarys_total_and_pick_are_the_numpy_statements():
    """dazim_map_tradeoff_total and dazim_tradeoff_pick are host code: the built library's functions on the reference's arrays, without
    a GPU; a NaN period makes that point's totals NaN and no other's"""
    import dazimsurftomo_amd as dz
    dz.build()
    prob, scale, damp, out = solved((9, 5), True, mref.REGS[0], 3)
    got, want = dz.map_tradeoff_total(out["mdata_p"], out["chi2"], out["reg2"], out["dof"], out["logev"]), ref.totals(out)
    for k in ref.TOTALS:
        assert np.abs(got[k] - want[k]).max() <= 1e-13 * max(1.0, np.abs(want[k]).max()), k
    part = dz.map_tradeoff_total(out["mdata_p"], out["chi2"], out["reg2"])
    assert part["dof"] is None and part["gcv"] is None and part["logev"] is None
    assert np.array_equal(part["chi2"], got["chi2"]) and np.array_equal(part["reg2sum"], got["reg2sum"])
    hole = {k: np.array(v, copy=True) for k, v in out.items()}
    for k in ("chi2", "reg2", "dof", "logev"):
        hole[k][2, 1] = np.nan
    got2 = dz.map_tradeoff_total(hole["mdata_p"], hole["chi2"], hole["reg2"], hole["dof"], hole["logev"])
    for k in ref.TOTALS:
        assert np.isnan(got2[k][2]) and np.array_equal(np.delete(got2[k], 2), np.delete(got[k], 2)), k
    reg2sum = out["reg2"].sum(axis=2)
    for p in range(3):
        assert dz.tradeoff_pick(out["chi2"][:, p], reg2sum[:, p], out["gcv"][:, p], out["logev"][:, p]) == \
            tref.pick(out["chi2"][:, p], reg2sum[:, p], out["gcv"][:, p], out["logev"][:, p])
    assert dz.tradeoff_pick(want["chi2"], want["reg2sum"], want["gcv"], want["logev"]) == \
        tref.pick(want["chi2"], want["reg2sum"], want["gcv"], want["logev"])
