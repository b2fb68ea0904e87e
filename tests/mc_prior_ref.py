"""NumPy restatement of the Monte-Carlo step of dazim_mc with the Gaussian smoothness prior of dazim_mc_set_prior (include/dazim.h,
DESIGN.md section 14): tests/mc_ref.py's step with E + Q in place of E wherever a decision is taken, E the energy of mc_ref (chi2, or
X(chi2) in noise mode) and Q = s2 |L d|^2 + d2 |d|^2 the prior energy of the state's knots about the reference.  Philox, the draws,
chi2, the energy, the proposals and the final statistics are mc_ref's; everything the prior does not touch is restated as there, so
that with the prior off the step returns what mc_ref.step returns."""
import numpy as np

from tests import mc_ref
from tests.mc_ref import BRANCHES, COV_MIN, block, chi2, cholesky, covariance, energy, layout, ndata, pairs, uniform


def prior_q(v, vref, smooth, damp):
    """Q of the columns of v [nlay][ncol] fp32 about vref [nlay][ncol] fp32, in the library's order: d = (double)v - (double)vref,
    t_a = 2 d_a at both ends and (2 d_a - d_{a-1}) - d_{a+1} between them, q1 = sum t_a^2 and q2 = sum d_a^2 in knot order from 0.0,
    Q = s2 q1 + d2 q2 with s2, d2 the squares in fp64 of the fp32 smooth and damp"""
    s2 = float(np.float32(smooth)) * float(np.float32(smooth))
    d2 = float(np.float32(damp)) * float(np.float32(damp))
    n = v.shape[0]
    d = v.astype(np.float64) - vref.astype(np.float64)
    q1, q2 = np.zeros(v.shape[1]), np.zeros(v.shape[1])
    for a in range(n):
        t = 2.0 * d[a] if a in (0, n - 1) else (2.0 * d[a] - d[a - 1]) - d[a + 1]
        q1 = q1 + t * t
        q2 = q2 + d[a] * d[a]
    return s2 * q1 + d2 * q2


def empty_prior(smooth, damp, vref, cur):
    """the prior record of a handle whose states are cur [nz][ncol]: vref [nlay][ncol] fp32 per column"""
    nlay = vref.shape[0]
    return dict(smooth=float(np.float32(smooth)), damp=float(np.float32(damp)), vref=vref, q=prior_q(cur[:nlay], vref, smooth, damp))


def step(st, tp, cov, ns, pr, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cobs, wdat, nbin, seed):
    """mc_ref.step with the prior record `pr` (empty_prior(), or MonteCarlo.prior_state() with vref per column; None: the prior is
    off).  Returns mc_ref.step's eight values, then the new prior record (None when off) and {"dec": decisions, "swap": swap rules
    that came out otherwise than the energies alone would have made them}."""
    nz, ncol = prop.shape
    nlay = nz - 1
    nt, nswap, beta = tp["ntemp"], tp["nswap"], tp["beta"]
    ncold = nchain // nt
    ncs, cs, rung, gid = layout(ncol, nchain, nt, gcell)
    if ns is None:
        X = lambda c2, sel=slice(None): c2
    else:
        a = float(np.float32(ns["a0"])) + 0.5 * ndata(wdat)            # [ncol]
        X = lambda c2, sel=slice(None): energy(c2, a[sel], ns["b0"])
    chi2p = chi2(pv, cobs, wdat)
    qp = prior_q(prop[:nlay], pr["vref"], pr["smooth"], pr["damp"]) if pr is not None else None
    diff = dict(dec=0, swap=0)
    first = t == 1
    if first:
        acc = np.ones(ncol, bool)
    else:
        c = st["chi2"]
        u = uniform(block(t, gid, 0, seed)[..., 0])
        with np.errstate(invalid="ignore"):
            alone = np.where(np.isinf(c), ~np.isinf(chi2p), np.log(u) < -0.5 * beta[rung] * (X(chi2p) - X(c)))
            if pr is None:
                acc = alone
            else:
                acc = np.where(np.isinf(c), ~np.isinf(chi2p), np.log(u) < -0.5 * beta[rung] * ((X(chi2p) + qp) - (X(c) + pr["q"])))
                diff["dec"] = int((acc != alone).sum())
    cur = st["cur"].copy()
    cur[:nlay, acc] = prop[:nlay, acc]
    ch2 = np.where(acc, chi2p, st["chi2"])
    q = np.where(acc, qp, pr["q"]) if pr is not None else None
    # the scale and the window of every (cell, rung)
    scale = tp["scale"].copy()
    acc_win = acc_win.copy()
    set0 = cov["cov_set"].copy() if cov is not None else np.zeros(ncs, np.int32)
    root = np.sqrt(np.float32(nlay))
    if not record:
        if not first:
            np.add.at(acc_win, (cs, rung), acc.astype(np.int64))
        if adapt:
            rate = acc_win.astype(np.float64) / (float(nadapt) * float(ncold))
            s = np.where(rate > 0.40, scale * np.float32(1.25), np.where(rate < 0.20, scale / np.float32(1.25), scale)).astype(np.float32)
            cap = np.where(set0 == 1, np.float32(2.0) / root, np.float32(0.5)).astype(np.float32)[:, None]
            scale = np.minimum(np.maximum(s, np.float32(1e-3)), cap).astype(np.float32)
            acc_win[:] = 0
    # the swap round, on the energies plus Q
    swap_try, swap_acc = tp["swap_try"].copy(), tp["swap_acc"].copy()
    seen = dict.fromkeys(BRANCHES, 0)
    if nt > 1 and not first and t % nswap == 0:
        w = t // nswap
        cl = np.nonzero((rung % 2 == w % 2) & (rung + 1 < nt))[0]
        cu = cl + 1
        u = uniform(block(t, gid[cl], 0, seed)[..., 1])
        ca, cb = ch2[cl], ch2[cu]
        both = ~np.isinf(ca) & ~np.isinf(cb)
        with np.errstate(invalid="ignore"):
            D = 0.5 * (beta[rung[cl]] - beta[rung[cl] + 1]) * (X(ca, cl) - X(cb, cl))
            alone = np.where(both, np.log(u) < D, np.isinf(ca) & ~np.isinf(cb))
            if pr is None:
                sw = alone
            else:
                D = 0.5 * (beta[rung[cl]] - beta[rung[cl] + 1]) * ((X(ca, cl) + q[cl]) - (X(cb, cl) + q[cu]))
                sw = np.where(both, np.log(u) < D, np.isinf(ca) & ~np.isinf(cb))
                diff["swap"] = int((sw != alone).sum())
        for name, m in zip(BRANCHES, (both, np.isinf(ca) & ~np.isinf(cb), ~np.isinf(ca) & np.isinf(cb), np.isinf(ca) & np.isinf(cb))):
            seen[name] = int(m.sum())
        l, h = cl[sw], cu[sw]
        cur[:nlay, l], cur[:nlay, h] = cur[:nlay, h].copy(), cur[:nlay, l].copy()
        ch2[l], ch2[h] = ch2[h].copy(), ch2[l].copy()
        if pr is not None:
            q[l], q[h] = q[h].copy(), q[l].copy()
        np.add.at(swap_try, (cs[cl], rung[cl]), 1)
        np.add.at(swap_acc, (cs[cl], rung[cl]), sw.astype(np.int64))
    # the records: the rung-0 chains; the best model over every chain, by raw chi2
    sums, hist, accepted = st["sums"].copy(), st["hist"].copy(), st["accepted"].copy()
    best, best_chi2 = st["best"].copy(), st["best_chi2"].copy()
    cold = rung == 0
    if record:
        if not first:
            accepted += acc & cold
        c2 = ch2.reshape(ncs, nchain)
        win = np.argmin(c2, axis=1)
        m = c2[np.arange(ncs), win]
        upd = m < best_chi2
        wcol = np.arange(ncs) * nchain + win
        best[:, upd] = cur[:nlay, wcol[upd]]
        best_chi2 = np.where(upd, m, best_chi2)
        v = cur[:nlay, cold].astype(np.float64)
        sums[0][:, cold] += v
        sums[1][:, cold] += v * v
        b = ((v - lo[:, cold]) / (hi[:, cold] - lo[:, cold]) * float(nbin)).astype(np.int64)
        b = np.clip(b, 0, nbin - 1)
        for k in range(nlay):
            np.add.at(hist, (cs[cold], k, b[k]), 1)
        if ns is not None:
            nsum, ncnt = ns["nsum"].copy(), ns["ncnt"].copy()
            rec = cold & ~np.isinf(ch2)
            B = float(np.float32(ns["b0"])) + 0.5 * ch2[rec]
            nsum[0, rec] += np.sqrt(B)
            nsum[1, rec] += B
            ncnt[rec] += 1
            ns = dict(ns, nsum=nsum, ncnt=ncnt)
    # kind 1: the sums over the rung-0 chains in chain order, the factor at an adaptation point
    factored = {}
    if cov is not None:
        cov = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cov.items()}
        if not record and not first:
            u = (cur[:nlay].astype(np.float64) - lo) / (hi - lo)
            pa, pc = pairs(nlay)
            for col in np.nonzero(cold)[0]:
                cov["cov_s1"][cs[col]] += u[:, col]
                cov["cov_s2"][cs[col]] += u[pa, col] * u[pc, col]
            cov["cov_n"] += ncold
            if adapt:
                for e in range(ncs):
                    if cov["cov_n"][e] < COV_MIN * nlay:
                        continue
                    Cm = covariance(cov["cov_n"][e], cov["cov_s1"][e], cov["cov_s2"][e], nlay)
                    ok, L = cholesky(Cm)
                    factored[e] = Cm
                    if ok:
                        cov["chol"][e] = L
                        if set0[e] == 0:
                            cov["cov_set"][e] = 1
                            scale[e, :] = np.float32(1.0) / root
                    cov["cov_n"][e] = 0
                    cov["cov_s1"][e] = 0.0
                    cov["cov_s2"][e] = 0.0
    new = dict(cur=cur, chi2=ch2, scale=scale[:, 0].copy(), step=t, sums=sums, hist=hist, accepted=accepted, best=best, best_chi2=best_chi2)
    ntp = dict(tp, scale=scale, swap_try=swap_try, swap_acc=swap_acc)
    npr = dict(pr, q=q) if pr is not None else None
    return new, ntp, cov, ns, acc, acc_win, factored, seen, npr, diff


proposals = mc_ref.proposals
final = mc_ref.final
