"""The drive-and-compare loop of the GPU step tests of dazim_mc (tests/test_column_mc_gpu.py, .._cov_gpu.py, .._temper_gpu.py,
.._noise_gpu.py, .._prior_gpu.py, .._groups_gpu.py): every step of a handle restated by tests/mc_ref.py from the library's own state,
in whatever modes the handle has."""
import numpy as np

from tests import mc_ref
from tests.mc_prior_ref import prior_q

STATE = ("cur", "chi2", "scale", "sums", "hist", "accepted", "best", "best_chi2")


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def snapshot(mc, vref=None):
    """(state, ladder, cov or None for kind 0, noise record or None for the fixed level, prior record or None) as mc_ref.step takes
    them: the single-scale record where set_noise's is on, else the groups' record; vref [nlay][ncol] the prior's centre per column"""
    st, cov, ns, ps = mc.state(), mc.cov_state(), mc.noise_state(), mc.prior_state()
    if "nsum" not in ns:
        ns = mc.noise_groups_state()
        ns = ns if ns["ngroup"] else None
    pr = dict(smooth=ps["smooth"], damp=ps["damp"], vref=vref, q=ps["q"]) if "q" in ps else None
    return st, mc_ref.ladder_state(st, mc.temper_state()), cov if cov["kind"] == 1 else None, ns, pr


def drive(mc, forward, nburn, nrec, nadapt, lo, hi, cb, wd, nbin, seed, moved=False, vref=None):
    """nburn + nrec steps on the curves forward(t), the same on both sides: the state, the ladder, the covariance sums and the noise
    record (nsum, ncnt, and chi2g as noise_groups_state() gives it) bit for bit, the factor to 1e-9 (fp64 epsilon times the condition
    number, <= 1e6 from the restatement alone, with a margin of ten), the next proposals, formed from the library's factor, within
    one fp32 ulp and inside the box; a state's chi2_g are +inf where its total is, and only there; with the prior (vref [nlay][ncol]
    its centre per column) prior_state()'s q bit for bit against the restated step's and against Q restated from the new states.
    moved: without swaps a moved state is an accepted proposal, so the decisions themselves are compared too.  Returns the last
    state, ladder, cov, noise and prior record (got, gtp, gcov, gns, gpr) and what the run went through: seen (the swap rule's
    cases), ninf0 (chains at chi2 = +inf after step 1), ndec (accepted decisions), nfact, conds and first_factor_at (in burn-in
    decisions), before / after (cells without / with a factor, summed over the steps with a decision), ninf_group (states with
    exactly one group at +inf), ndiff_dec / ndiff_swap (decisions and swap rules that the energies alone would have taken otherwise)."""
    nlay, nchain = mc.nlay, mc.nchain
    root = np.sqrt(np.float32(nlay))
    acc_win = np.zeros((mc.ncs, mc.temper_state()["ntemp"]), np.int64)
    out = dict(seen=dict.fromkeys(mc_ref.BRANCHES, 0), ninf0=0, ndec=0, nfact=0, conds=[], first_factor_at=None, before=0, after=0,
               ninf_group=0, ndiff_dec=0, ndiff_swap=0)
    nbd = 0
    for t in range(1, nburn + nrec + 1):
        st, tp, cov, ns, pr = snapshot(mc, vref)
        assert st["step"] == t - 1
        prop = mc.proposals().cpu().numpy()
        record = t > nburn
        adapt = False
        if not record and t > 1:
            nbd += 1
            adapt = nbd % nadapt == 0
        pv = forward(t)
        e = mc_ref.step(st, tp, cov, ns, pr, prop, pv, t, record, adapt, nadapt, acc_win, mc._cells, nchain, lo, hi, cb, wd, nbin, seed)
        exp, etp, ecov, ens, epr, acc, acc_win, factored = (e[k] for k in ("st", "tp", "cov", "ns", "pr", "acc", "acc_win", "factored"))
        for k in e["seen"]:
            out["seen"][k] += e["seen"][k]
        out["ndiff_dec"] += e["diff"]["dec"]
        out["ndiff_swap"] += e["diff"]["swap"]
        if cov is not None and t > 1:
            out["before"] += int((cov["cov_set"] == 0).sum())
            out["after"] += int((cov["cov_set"] == 1).sum())
        mc.step(pv, int(record))
        got, gtp, gcov, gns, gpr = snapshot(mc, vref)
        gprop = mc.proposals().cpu().numpy()
        if moved:
            mv = (got["cur"][:nlay] == prop[:nlay]).all(axis=0) & ((got["cur"][:nlay] != st["cur"][:nlay]).any(axis=0) | (t == 1))
            assert np.array_equal(mv, acc), t
        for k in STATE:
            assert np.array_equal(got[k], exp[k]), (t, k)
        for k in ("scale", "swap_try", "swap_acc"):
            assert np.array_equal(gtp[k], etp[k]), (t, k)
        assert np.array_equal(got["scale"], gtp["scale"][:, 0]), t
        if pr is not None:
            assert np.array_equal(gpr["q"], epr["q"]), t
            assert np.array_equal(gpr["q"], prior_q(got["cur"][:nlay], vref, pr["smooth"], pr["damp"])), t
        if ns is not None:
            for k in ("nsum", "ncnt"):
                assert np.array_equal(gns[k], ens[k]), (t, k)
            cg = mc.noise_groups_state()["chi2g"]               # (the single scale's too: its one group's chi2_g is chi2)
            assert np.array_equal(cg, mc_ref.as_groups(ens, exp["chi2"], cb.shape[0])["chi2g"]), t
            # a state's chi2_g are +inf where its total is, and only there
            assert np.array_equal(np.isinf(cg).any(axis=0), np.isinf(got["chi2"])), t
            out["ninf_group"] += int((np.isinf(cg).sum(axis=0) == 1).sum())
        if cov is not None:
            for k in ("cov_n", "cov_s1", "cov_s2", "cov_set"):
                assert np.array_equal(gcov[k], ecov[k]), (t, k)
            for cs, Cm in factored.items():
                out["conds"].append(np.linalg.cond(Cm))
                assert out["conds"][-1] <= 1e6, (t, cs, out["conds"][-1])   # from the restatement alone: the bound below rests on it
                out["nfact"] += 1
                if out["first_factor_at"] is None:
                    out["first_factor_at"] = nbd
                if cov["cov_set"][cs] == 0:                 # the first factor: every rung's scale restarts, whatever the rule made of it
                    assert gcov["cov_set"][cs] == 1 and (gtp["scale"][cs] == np.float32(1.0) / root).all()
            assert np.abs(gcov["chol"] - ecov["chol"]).max() <= 1e-9 * np.abs(ecov["chol"]).max(), t
        nxt = mc_ref.proposals(got["cur"], gtp["scale"], gcov, prop, t, mc._cells, nchain, lo, hi, seed)
        assert ulps(gprop, nxt).max() <= 1, (t, ulps(gprop, nxt).max())
        assert (gprop[:nlay] >= lo).all() and (gprop[:nlay] <= hi).all()
        if t == 1:
            out["ninf0"] = int(np.isinf(got["chi2"]).sum())
        else:
            out["ndec"] += int(acc.sum())
    out.update(got=got, gtp=gtp, gcov=gcov, gns=gns, gpr=gpr)
    return out


def check_final(mc, got, vmin, vmax, vel0, ntemp, nrec, nbin, roots=True):
    """dazim_mc_result of the nrec recorded steps against k_mc_final restated from the state `got`: mean, q, best, accept, chi2_best
    bit for bit and, with roots, std and rhat (sqrt in fp64, then fp32) equal or one fp32 ulp apart.  Returns the result and the
    smallest finite fraction of std and rhat in the restatement."""
    nlay, ncell = mc.nlay, (mc.ny - 2) * (mc.nx - 2)
    r = mc.result()
    e = mc_ref.final(got, vmin.reshape(nlay, ncell), vmax.reshape(nlay, ncell), vel0[:nlay, 1:-1, 1:-1].reshape(nlay, ncell),
                     mc._cells, ncell, mc.nchain, ntemp, nrec, nrec, nbin)
    for k in ("mean", "q", "best", "accept", "chi2_best"):
        assert np.array_equal(r[k].reshape(e[k].shape), e[k]), k
    finite = 1.0
    for k in ("std", "rhat") if roots else ():
        a, b = r[k].reshape(e[k].shape), e[k]
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), k
        if fin.any():
            assert ulps(a[fin], b[fin]).max() <= 1, k
        finite = min(finite, fin.mean())
    return r, finite
