"""NumPy restatement of the tempered Monte-Carlo step of dazim_mc ("Parallel tempering" in include/dazim.h) on
the pieces of tests/mc_ref.py and tests/mc_cov_ref.py: the decision at rung r, the scale per rung, the swaps, the records of the
rung-0 chains and, for proposal kind 1, the covariance sums over the rung-0 chains.  Every operation is the library's in the same
order and precision; only log, sqrt, cos and sin may differ in the last bit."""
import numpy as np

from tests import mc_cov_ref, mc_ref

BRANCHES = ("both_finite", "lower_inf", "upper_inf", "both_inf")


def ladder(ntemp, tmax):
    """beta_r = tmax^(-r / (ntemp - 1)), beta_0 = 1"""
    return np.array([1.0] + [float(tmax) ** (-r / (ntemp - 1)) for r in range(1, ntemp)])


def layout(ncol, nchain, ntemp, gcell):
    ncs = ncol // nchain
    cs = np.repeat(np.arange(ncs), nchain)
    ch = np.tile(np.arange(nchain), ncs)
    gid = (gcell[cs] * nchain + ch).astype(np.uint32)
    return ncs, cs, ch % ntemp, gid


def step(st, tp, cov, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cobs, wdat, nbin, seed):
    """one tempered step from the state `st` (MonteCarlo.state()), the ladder `tp` (MonteCarlo.temper_state()) and, for kind 1, `cov`
    (MonteCarlo.cov_state(); None for kind 0); acc_win [ncs][ntemp] the burn-in window counts; the other arguments are mc_ref.step's.
    Returns (new state, new ladder state, new cov with the restated factor or None, accept decisions [ncol], acc_win, {cs: C} of the
    cells factored in this step, {branch: pairs} of the swap rule's four cases).  The next proposals come from proposals()."""
    nz, ncol = prop.shape
    nlay = nz - 1
    nt, nswap, beta = tp["ntemp"], tp["nswap"], tp["beta"]
    ncold = nchain // nt
    ncs, cs, rung, gid = layout(ncol, nchain, nt, gcell)
    chi2p = mc_ref.chi2(pv, cobs, wdat)
    first = t == 1
    if first:
        acc = np.ones(ncol, bool)
    else:
        c = st["chi2"]
        u = mc_ref.uniform(mc_ref.block(t, gid, 0, seed)[..., 0])
        with np.errstate(invalid="ignore"):
            acc = np.where(np.isinf(c), ~np.isinf(chi2p), np.log(u) < -0.5 * beta[rung] * (chi2p - c))
    cur = st["cur"].copy()
    cur[:nlay, acc] = prop[:nlay, acc]
    ch2 = np.where(acc, chi2p, st["chi2"])
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
    # the swap round
    swap_try, swap_acc = tp["swap_try"].copy(), tp["swap_acc"].copy()
    seen = dict.fromkeys(BRANCHES, 0)
    if not first and t % nswap == 0:
        w = t // nswap
        cl = np.nonzero((rung % 2 == w % 2) & (rung + 1 < nt))[0]
        cu = cl + 1
        u = mc_ref.uniform(mc_ref.block(t, gid[cl], 0, seed)[..., 1])
        a, b = ch2[cl], ch2[cu]
        with np.errstate(invalid="ignore"):
            D = 0.5 * (beta[rung[cl]] - beta[rung[cl] + 1]) * (a - b)
            sw = np.where(~np.isinf(a) & ~np.isinf(b), np.log(u) < D, np.isinf(a) & ~np.isinf(b))
        for name, m in zip(BRANCHES, (~np.isinf(a) & ~np.isinf(b), np.isinf(a) & ~np.isinf(b), ~np.isinf(a) & np.isinf(b),
                                      np.isinf(a) & np.isinf(b))):
            seen[name] = int(m.sum())
        l, h = cl[sw], cu[sw]
        cur[:nlay, l], cur[:nlay, h] = cur[:nlay, h].copy(), cur[:nlay, l].copy()
        ch2[l], ch2[h] = ch2[h].copy(), ch2[l].copy()
        np.add.at(swap_try, (cs[cl], rung[cl]), 1)
        np.add.at(swap_acc, (cs[cl], rung[cl]), sw.astype(np.int64))
    # the records: the rung-0 chains; the best model over every chain
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
    # kind 1: the sums over the rung-0 chains in chain order, the factor at an adaptation point
    factored = {}
    if cov is not None:
        cov = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cov.items()}
        if not record and not first:
            u = (cur[:nlay].astype(np.float64) - lo) / (hi - lo)
            a, c = mc_cov_ref.pairs(nlay)
            for col in np.nonzero(cold)[0]:
                cov["cov_s1"][cs[col]] += u[:, col]
                cov["cov_s2"][cs[col]] += u[a, col] * u[c, col]
            cov["cov_n"] += ncold
            if adapt:
                for e in range(ncs):
                    if cov["cov_n"][e] < mc_cov_ref.COV_MIN * nlay:
                        continue
                    C = mc_cov_ref.covariance(cov["cov_n"][e], cov["cov_s1"][e], cov["cov_s2"][e], nlay)
                    ok, L = mc_cov_ref.cholesky(C)
                    factored[e] = C
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
    return new, ntp, cov, acc, acc_win, factored, seen


def proposals(cur, tscale, cov, prop, t, gcell, nchain, lo, hi, seed):
    """the proposals after step t from the state cur [nz][ncol], the scales tscale [ncs][ntemp] and, for kind 1, cov's packed factors
    chol [ncs][npair] and cov_set (None for kind 0)"""
    nz, ncol = prop.shape
    nlay = nz - 1
    ncs, cs, rung, gid = layout(ncol, nchain, tscale.shape[1], gcell)
    z = mc_ref.normals(t, gid, nlay, seed)
    y = z.copy()
    if cov is not None:
        on = cov["cov_set"][cs] == 1
        for k in range(nlay):
            yk = np.zeros(ncol)
            for j in range(k + 1):
                yk = yk + cov["chol"][cs, k * (k + 1) // 2 + j] * z[j]
            y[k] = np.where(on, yk, z[k])
    d = tscale[cs, rung].astype(np.float64) * (hi - lo)
    v = cur[:nlay].astype(np.float64) + d * y
    for _ in range(mc_ref.MAXFOLD):
        below, above = v < lo, v > hi
        if not (below | above).any():
            break
        v = np.where(below, 2.0 * lo - v, np.where(above, 2.0 * hi - v, v))
    nxt = prop.copy()
    nxt[:nlay] = np.minimum(np.maximum(v, lo), hi).astype(np.float32)
    return nxt


def final(st, vmin, vmax, vel0_knots, cells, ncell, nchain, ntemp, nrec, ndec, nbin):
    """dazim_mc_result of a tempered handle: mc_ref.final over the rung-0 chains with M = ncold.  For ncold = 1 the one chain is handed
    over twice, which scales every sum, count and total by an exact 2 and so leaves the quotients' bits alone, and R-hat is NaN."""
    ncold = nchain // ntemp
    ncs = st["accepted"].size // nchain
    cold = (np.arange(ncs * nchain) % nchain) % ntemp == 0
    rep = 2 if ncold == 1 else 1
    sub = dict(st, sums=np.repeat(st["sums"][:, :, cold], rep, axis=2), accepted=np.repeat(st["accepted"][cold], rep),
               hist=st["hist"] * rep)
    out = mc_ref.final(sub, vmin, vmax, vel0_knots, cells, ncell, ncold * rep, nrec, ndec, nbin)
    if ncold == 1:
        out["rhat"][:] = np.nan
    return out
