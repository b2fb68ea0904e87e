"""NumPy restatement of the Monte-Carlo step of dazim_mc with the hierarchical data-noise scale ("Hierarchical data noise" in
include/dazim.h) on the pieces of tests/mc_ref.py, tests/mc_cov_ref.py and tests/mc_pt_ref.py: the energy
X = 2 a log(b0 + chi2 / 2) wherever a decision is taken, the noise record of the rung-0 chains and the result.  One step function
serves both proposal kinds, tempered or not (an untempered handle is a ladder of one rung with beta = 1, which leaves every product
unchanged).  Every operation is the library's in the same order and precision; only log, sqrt, cos and sin may differ in the last
bit, and lgamma and exp of the result's table in the last few."""
import math

import numpy as np

from tests import mc_cov_ref, mc_pt_ref, mc_ref

BRANCHES = mc_pt_ref.BRANCHES


def ndata(wdat):
    """periods with data per column (wdat [kmax][ncol]) or per cell (wdat [kmax][ncell])"""
    return (wdat != 0).sum(axis=0)


def energy(chi2, a, b0):
    """X = 2 a log(B(chi2)), B = (double)b0 + chi2 / 2; +inf at chi2 = +inf"""
    with np.errstate(invalid="ignore"):
        return 2.0 * a * np.log(float(np.float32(b0)) + 0.5 * chi2)


def ladder_state(st, tp):
    """the ladder of a handle as mc_pt_ref holds it; an untempered handle (temper_state() without arrays) is one rung at beta 1"""
    if tp["ntemp"] > 1:
        return tp
    ncs = st["scale"].size
    return dict(tp, beta=np.array([1.0]), scale=st["scale"].reshape(ncs, 1).copy(), swap_try=np.zeros((ncs, 0), np.int64),
                swap_acc=np.zeros((ncs, 0), np.int64))


def empty_noise(a0, b0, ncol):
    return dict(a0=float(np.float32(a0)), b0=float(np.float32(b0)), nsum=np.zeros((2, ncol)), ncnt=np.zeros(ncol, np.int64))


def step(st, tp, cov, ns, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cobs, wdat, nbin, seed):
    """one step from the state `st` (MonteCarlo.state()), the ladder `tp` (ladder_state()), `cov` (MonteCarlo.cov_state() for kind 1,
    None for kind 0) and the noise record `ns` (MonteCarlo.noise_state()); acc_win [ncs][ntemp]; the other arguments are
    mc_ref.step's.  Returns (new state, new ladder state, new cov or None, new noise record, accept decisions [ncol], acc_win,
    {cs: C} of the cells factored in this step, {branch: pairs} of the swap rule's cases).  mc_pt_ref.proposals() gives the next
    proposals."""
    nz, ncol = prop.shape
    nlay = nz - 1
    nt, nswap, beta = tp["ntemp"], tp["nswap"], tp["beta"]
    ncold = nchain // nt
    ncs, cs, rung, gid = mc_pt_ref.layout(ncol, nchain, nt, gcell)
    a = float(np.float32(ns["a0"])) + 0.5 * ndata(wdat)            # [ncol]
    b0 = ns["b0"]
    chi2p = mc_ref.chi2(pv, cobs, wdat)
    first = t == 1
    if first:
        acc = np.ones(ncol, bool)
    else:
        c = st["chi2"]
        u = mc_ref.uniform(mc_ref.block(t, gid, 0, seed)[..., 0])
        with np.errstate(invalid="ignore"):
            acc = np.where(np.isinf(c), ~np.isinf(chi2p), np.log(u) < -0.5 * beta[rung] * (energy(chi2p, a, b0) - energy(c, a, b0)))
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
    # the swap round, on the energies
    swap_try, swap_acc = tp["swap_try"].copy(), tp["swap_acc"].copy()
    seen = dict.fromkeys(BRANCHES, 0)
    if nt > 1 and not first and t % nswap == 0:
        w = t // nswap
        cl = np.nonzero((rung % 2 == w % 2) & (rung + 1 < nt))[0]
        cu = cl + 1
        u = mc_ref.uniform(mc_ref.block(t, gid[cl], 0, seed)[..., 1])
        ca, cb = ch2[cl], ch2[cu]
        with np.errstate(invalid="ignore"):
            D = 0.5 * (beta[rung[cl]] - beta[rung[cl] + 1]) * (energy(ca, a[cl], b0) - energy(cb, a[cl], b0))
            sw = np.where(~np.isinf(ca) & ~np.isinf(cb), np.log(u) < D, np.isinf(ca) & ~np.isinf(cb))
        for name, m in zip(BRANCHES, (~np.isinf(ca) & ~np.isinf(cb), np.isinf(ca) & ~np.isinf(cb), ~np.isinf(ca) & np.isinf(cb),
                                      np.isinf(ca) & np.isinf(cb))):
            seen[name] = int(m.sum())
        l, h = cl[sw], cu[sw]
        cur[:nlay, l], cur[:nlay, h] = cur[:nlay, h].copy(), cur[:nlay, l].copy()
        ch2[l], ch2[h] = ch2[h].copy(), ch2[l].copy()
        np.add.at(swap_try, (cs[cl], rung[cl]), 1)
        np.add.at(swap_acc, (cs[cl], rung[cl]), sw.astype(np.int64))
    # the records: the rung-0 chains; the best model over every chain, by raw chi2
    sums, hist, accepted = st["sums"].copy(), st["hist"].copy(), st["accepted"].copy()
    best, best_chi2 = st["best"].copy(), st["best_chi2"].copy()
    nsum, ncnt = ns["nsum"].copy(), ns["ncnt"].copy()
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
        # the noise record: B at the state of every rung-0 chain with a finite chi2
        rec = cold & ~np.isinf(ch2)
        B = float(np.float32(b0)) + 0.5 * ch2[rec]
        nsum[0, rec] += np.sqrt(B)
        nsum[1, rec] += B
        ncnt[rec] += 1
    # kind 1: the sums over the rung-0 chains in chain order, the factor at an adaptation point
    factored = {}
    if cov is not None:
        cov = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cov.items()}
        if not record and not first:
            u = (cur[:nlay].astype(np.float64) - lo) / (hi - lo)
            pa, pc = mc_cov_ref.pairs(nlay)
            for col in np.nonzero(cold)[0]:
                cov["cov_s1"][cs[col]] += u[:, col]
                cov["cov_s2"][cs[col]] += u[pa, col] * u[pc, col]
            cov["cov_n"] += ncold
            if adapt:
                for e in range(ncs):
                    if cov["cov_n"][e] < mc_cov_ref.COV_MIN * nlay:
                        continue
                    Cm = mc_cov_ref.covariance(cov["cov_n"][e], cov["cov_s1"][e], cov["cov_s2"][e], nlay)
                    ok, L = mc_cov_ref.cholesky(Cm)
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
    return new, ntp, cov, dict(ns, nsum=nsum, ncnt=ncnt), acc, acc_win, factored, seen


def gamma_ratio(a):
    """g(a) = Gamma(a - 1/2) / Gamma(a) as the library's table forms it"""
    return math.exp(math.lgamma(a - 0.5) - math.lgamma(a))


def result(ns, wdat_cells, cells, ncell, nchain, ntemp):
    """dazim_mc_noise_result from a noise record: wdat_cells [kmax][ncell] fp32 (the inner cells), cells the sampled inner-cell
    indices.  Returns dict lam_mean, lam_std [ncell] fp32 and ndata [ncell] int32."""
    nd = ndata(wdat_cells).astype(np.int32)
    lam_mean, lam_std = np.zeros(ncell, np.float32), np.zeros(ncell, np.float32)
    a0 = float(np.float32(ns["a0"]))
    for cs, cell in enumerate(cells):
        n, s0, s1 = 0, 0.0, 0.0
        for ch in range(0, nchain, ntemp):
            col = cs * nchain + ch
            n += int(ns["ncnt"][col])
            s0 += ns["nsum"][0, col]
            s1 += ns["nsum"][1, col]
        if n == 0:
            lam_mean[cell] = lam_std[cell] = np.nan
            continue
        a = a0 + 0.5 * int(nd[cell])
        lm = gamma_ratio(a) * s0 / float(n)
        lam_mean[cell] = np.float32(lm)
        lam_std[cell] = np.nan if a <= 1.0 else np.float32(math.sqrt(max(s1 / (float(n) * (a - 1.0)) - lm * lm, 0.0)))
    return dict(lam_mean=lam_mean, lam_std=lam_std, ndata=nd)


def sample(forward, nburn, nsample, nadapt, gcell, nchain, vmin, vmax, vlast, cobs, wdat, nbin, seed, a0, b0, step0=0.05, ntemp=1,
           tmax=1.0, nswap=1, kind=0):
    """the whole sampler from the restatement alone, no library: vmin, vmax [nlay][ncs], vlast [ncs], cobs, wdat [kmax][ncs] fp32 of
    the sampled cells gcell; forward(prop [nz][ncol] fp32) -> curves [kmax][ncol] fp64.  a0 = 0: the fixed noise level (the energy
    is chi2 itself).  Returns (state, ladder, noise record)."""
    nlay, ncs = vmin.shape
    ncol = ncs * nchain
    rep = lambda x: np.repeat(x, nchain, axis=-1)
    lo, hi = rep(vmin.astype(np.float64)), rep(vmax.astype(np.float64))
    cb, wd = rep(cobs), rep(wdat)
    _, _, _, gid = mc_pt_ref.layout(ncol, nchain, ntemp, gcell)
    prop = np.concatenate([mc_ref.start_models(gid, lo, hi, seed), rep(vlast.astype(np.float32))[None]])
    st = dict(cur=prop.copy(), chi2=np.full(ncol, np.inf), scale=np.full(ncs, step0, np.float32), step=0,
              sums=np.zeros((2, nlay, ncol)), hist=np.zeros((ncs, nlay, nbin), np.uint32), accepted=np.zeros(ncol, np.int64),
              best=np.zeros((nlay, ncs), np.float32), best_chi2=np.full(ncs, np.inf))
    tp = dict(ntemp=ntemp, tmax=tmax, nswap=nswap)
    if ntemp > 1:
        tp.update(beta=mc_pt_ref.ladder(ntemp, tmax), scale=np.full((ncs, ntemp), step0, np.float32),
                  swap_try=np.zeros((ncs, ntemp - 1), np.int64), swap_acc=np.zeros((ncs, ntemp - 1), np.int64))
    tp = ladder_state(st, tp)
    cov = mc_cov_ref.empty_cov(ncs, nlay) if kind == 1 else None
    ns = empty_noise(a0, b0, ncol)
    fixed = a0 == 0
    acc_win = np.zeros((ncs, ntemp), np.int64)
    nbd = 0
    for t in range(1, nburn + nsample + 1):
        record = t > nburn
        adapt = False
        if not record and t > 1:
            nbd += 1
            adapt = nbd % nadapt == 0
        pv = forward(prop)
        if fixed:
            st, tp, cov, _, acc_win, _, _ = mc_pt_ref.step(st, tp, cov, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo,
                                                           hi, cb, wd, nbin, seed)
        else:
            st, tp, cov, ns, _, acc_win, _, _ = step(st, tp, cov, ns, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo,
                                                     hi, cb, wd, nbin, seed)
        prop = mc_pt_ref.proposals(st["cur"], tp["scale"], cov, prop, t, gcell, nchain, lo, hi, seed)
    return st, tp, ns


def linear_problem(noise=0.06, sig=0.02, nsd=8.0, a0=2.0, b0=1.0, seed=5):
    """the linear problem of the noise tests: c = K v, 16 cells, 12 periods, 4 sampled knots, w = 1 / sig as fp32, data noise
    `noise`.  With lambda integrated out the posterior of v is a multivariate t: nu = 2 a0 + nd - p, mean the least-squares mu,
    covariance (2 b0 + chi2_min) / (nu - 2) P^-1, P = K^T K w^2; lambda^2 ~ IG(a0 + (nd - p) / 2, b0 + chi2_min / 2).  The box is
    mu +- nsd of those std."""
    rng = np.random.default_rng(seed)
    ncell, kmax, nlay = 16, 12, 4
    K = np.vstack([np.eye(nlay)] * 3) + 0.35 * rng.random((kmax, nlay))
    w32 = float(np.float32(1.0 / sig))
    vtrue = rng.uniform(3.0, 4.0, (ncell, nlay))
    cobs = (vtrue @ K.T + rng.normal(0, noise, (ncell, kmax))).astype(np.float32)
    P = K.T @ K * w32 ** 2
    Pinv = np.linalg.inv(P)
    mu = (cobs.astype(np.float64) @ K * w32 ** 2) @ Pinv          # [ncell][nlay]
    res = cobs.astype(np.float64) - mu @ K.T
    chi2_min = ((w32 * res) ** 2).sum(axis=1)                     # [ncell]
    nu = 2.0 * a0 + kmax - nlay
    sd = np.sqrt((2.0 * b0 + chi2_min)[:, None] / (nu - 2.0) * np.diag(Pinv)[None, :])
    sd_fixed = np.sqrt(np.diag(Pinv))
    alpha, beta = a0 + 0.5 * (kmax - nlay), b0 + 0.5 * chi2_min
    lam1 = np.sqrt(beta) * gamma_ratio(alpha)
    lam2 = beta / (alpha - 1.0)
    return dict(K=K, cobs=cobs, mu=mu, sd=sd, sd_fixed=sd_fixed, lam_mean=lam1, lam_std=np.sqrt(lam2 - lam1 ** 2),
                vmin=(mu - nsd * sd).astype(np.float32), vmax=(mu + nsd * sd).astype(np.float32), w=np.float32(1.0 / sig),
                ncell=ncell, kmax=kmax, nlay=nlay, a0=a0, b0=b0)
