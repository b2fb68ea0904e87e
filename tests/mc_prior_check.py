"""The drive-and-compare loop of tests/test_column_mc_prior_gpu.py: tests/mc_step_check.drive for a handle with the Gaussian prior of
dazim_mc_set_prior on, every step restated by tests/mc_prior_ref.py from the library's own state."""
import numpy as np

from tests import mc_prior_ref, mc_ref
from tests.mc_step_check import STATE, snapshot, ulps


def prior_snapshot(mc, vref_col):
    """the prior record as mc_prior_ref.step takes it (vref per column), or None while the prior is off"""
    ps = mc.prior_state()
    return dict(smooth=ps["smooth"], damp=ps["damp"], vref=vref_col, q=ps["q"]) if "q" in ps else None


def drive(mc, forward, nburn, nrec, nadapt, lo, hi, cb, wd, vref_col, nbin, seed):
    """mc_step_check.drive's comparisons, and beside them the prior energies: prior_state()'s q bit for bit against the restated
    step's, and against Q restated from the new states themselves.  Returns mc_step_check.drive's dict with the prior record (gpr)
    and ndiff_dec / ndiff_swap: the decisions and the swap rules that the energies alone would have taken otherwise."""
    nlay, nchain = mc.nlay, mc.nchain
    root = np.sqrt(np.float32(nlay))
    acc_win = np.zeros((mc.ncs, mc.temper_state()["ntemp"]), np.int64)
    out = dict(seen=dict.fromkeys(mc_ref.BRANCHES, 0), ninf0=0, ndec=0, nfact=0, conds=[], ndiff_dec=0, ndiff_swap=0)
    nbd = 0
    for t in range(1, nburn + nrec + 1):
        st, tp, cov, ns = snapshot(mc)
        pr = prior_snapshot(mc, vref_col)
        assert st["step"] == t - 1
        prop = mc.proposals().cpu().numpy()
        record = t > nburn
        adapt = False
        if not record and t > 1:
            nbd += 1
            adapt = nbd % nadapt == 0
        pv = forward(t)
        exp, etp, ecov, ens, acc, acc_win, factored, br, epr, diff = mc_prior_ref.step(
            st, tp, cov, ns, pr, prop, pv, t, record, adapt, nadapt, acc_win, mc._cells, nchain, lo, hi, cb, wd, nbin, seed)
        for k in br:
            out["seen"][k] += br[k]
        out["ndiff_dec"] += diff["dec"]
        out["ndiff_swap"] += diff["swap"]
        mc.step(pv, int(record))
        got, gtp, gcov, gns = snapshot(mc)
        gpr = prior_snapshot(mc, vref_col)
        gprop = mc.proposals().cpu().numpy()
        for k in STATE:
            assert np.array_equal(got[k], exp[k]), (t, k)
        for k in ("scale", "swap_try", "swap_acc"):
            assert np.array_equal(gtp[k], etp[k]), (t, k)
        assert np.array_equal(got["scale"], gtp["scale"][:, 0]), t
        if pr is not None:
            assert np.array_equal(gpr["q"], epr["q"]), t
            assert np.array_equal(gpr["q"], mc_prior_ref.prior_q(got["cur"][:nlay], vref_col, pr["smooth"], pr["damp"])), t
        if ns is not None:
            for k in ("nsum", "ncnt"):
                assert np.array_equal(gns[k], ens[k]), (t, k)
        if cov is not None:
            for k in ("cov_n", "cov_s1", "cov_s2", "cov_set"):
                assert np.array_equal(gcov[k], ecov[k]), (t, k)
            for cs, Cm in factored.items():
                out["conds"].append(np.linalg.cond(Cm))
                assert out["conds"][-1] <= 1e6, (t, cs, out["conds"][-1])
                out["nfact"] += 1
                if cov["cov_set"][cs] == 0:
                    assert gcov["cov_set"][cs] == 1 and (gtp["scale"][cs] == np.float32(1.0) / root).all()
            assert np.abs(gcov["chol"] - ecov["chol"]).max() <= 1e-9 * np.abs(ecov["chol"]).max(), t
        nxt = mc_prior_ref.proposals(got["cur"], gtp["scale"], gcov, prop, t, mc._cells, nchain, lo, hi, seed)
        assert ulps(gprop, nxt).max() <= 1, (t, ulps(gprop, nxt).max())
        assert (gprop[:nlay] >= lo).all() and (gprop[:nlay] <= hi).all()
        if t == 1:
            out["ninf0"] = int(np.isinf(got["chi2"]).sum())
        else:
            out["ndec"] += int(acc.sum())
    out.update(got=got, gtp=gtp, gcov=gcov, gns=gns, gpr=gpr)
    return out
