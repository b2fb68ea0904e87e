"""NumPy restatement of the Monte-Carlo step with one noise scale per group of periods (dazim_mc_set_noise_groups, include/dazim.h,
DESIGN.md section 14): chi2_g beside chi2, the energy X = sum_g 2 a_g log(b0_g + chi2_g / 2), the record per group and its result.
Everything the groups do not touch is tests/mc_ref.py's: the random numbers, the proposals, the ladder, the covariance sums and the Vs
statistics.  With one group every function here returns the bytes of its mc_ref counterpart (tests/test_mc_groups_ref_cpu.py)."""
import math

import numpy as np

from tests import mc_ref
from tests.mc_ref import BRANCHES, COV_MIN, block, cholesky, covariance, layout, pairs, uniform

MAXGRP = 4


def chi2_groups(pv, cobs, wdat, grp, G):
    """the total chi2 [ncol] as mc_ref.chi2 forms it and chi2_g [G][ncol], each in period order within its group; a period with
    data and no root makes the total and its group +inf"""
    kmax, ncol = pv.shape
    s, sg = np.zeros(ncol), np.zeros((G, ncol))
    for p in range(kmax):
        r = wdat[p].astype(np.float64) * (cobs[p].astype(np.float64) - pv[p])
        rr = r * r
        data, noroot = wdat[p] != 0, pv[p] == 0.0
        s = np.where(data, np.where(noroot, np.inf, s + rr), s)
        sg[grp[p]] = np.where(data, np.where(noroot, np.inf, sg[grp[p]] + rr), sg[grp[p]])
    return s, sg


def ndata_groups(wdat, grp, G):
    """periods with data per group: [G][ncol] from wdat [kmax][ncol], or per cell from wdat [kmax][ncell]"""
    return np.array([((wdat != 0) & (np.asarray(grp)[:, None] == g)).sum(axis=0) for g in range(G)])


def energy_groups(c2, cg, ndg, a0, b0):
    """X [ncol] = sum over g in group order from 0.0, over the groups with nd_g > 0, of 2 a_g log(B_g); +inf where the total c2 is"""
    x = np.zeros(c2.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        for g in range(len(a0)):
            a = float(np.float32(a0[g])) + 0.5 * ndg[g]
            x = np.where(ndg[g] > 0, x + 2.0 * a * np.log(float(np.float32(b0[g])) + 0.5 * cg[g]), x)
    return np.where(np.isinf(c2), np.inf, x)


def empty_groups(grp, a0, b0, ncol):
    G = len(a0)
    return dict(ngroup=G, group_of_period=np.asarray(grp, np.int32).copy(), a0=np.asarray(a0, np.float32).copy(),
                b0=np.asarray(b0, np.float32).copy(), chi2g=np.full((G, ncol), np.inf), nsum=np.zeros((2, G, ncol)),
                ncnt=np.zeros(ncol, np.int64))


def step(st, tp, cov, gs, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cobs, wdat, nbin, seed):
    """mc_ref.step with the noise groups `gs` (MonteCarlo.noise_groups_state(), or empty_groups) in place of its noise record: the
    same arguments, the same returns with the new groups' state (chi2g, nsum, ncnt) fourth"""
    nz, ncol = prop.shape
    nlay = nz - 1
    nt, nswap, beta = tp["ntemp"], tp["nswap"], tp["beta"]
    ncold = nchain // nt
    ncs, cs, rung, gid = layout(ncol, nchain, nt, gcell)
    G, grp, a0, b0 = gs["ngroup"], gs["group_of_period"], gs["a0"], gs["b0"]
    ndg = ndata_groups(wdat, grp, G)
    chi2p, cgp = chi2_groups(pv, cobs, wdat, grp, G)
    first = t == 1
    if first:
        acc = np.ones(ncol, bool)
    else:
        c = st["chi2"]
        u = uniform(block(t, gid, 0, seed)[..., 0])
        xp, xc = energy_groups(chi2p, cgp, ndg, a0, b0), energy_groups(c, gs["chi2g"], ndg, a0, b0)
        with np.errstate(invalid="ignore"):
            acc = np.where(np.isinf(c), ~np.isinf(chi2p), np.log(u) < -0.5 * beta[rung] * (xp - xc))
    cur = st["cur"].copy()
    cur[:nlay, acc] = prop[:nlay, acc]
    ch2 = np.where(acc, chi2p, st["chi2"])
    cg = np.where(acc[None, :], cgp, gs["chi2g"])
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
    # the swap round, on the energies of the states; the chi2_g change columns with the knots and chi2
    swap_try, swap_acc = tp["swap_try"].copy(), tp["swap_acc"].copy()
    seen = dict.fromkeys(BRANCHES, 0)
    if nt > 1 and not first and t % nswap == 0:
        w = t // nswap
        cl = np.nonzero((rung % 2 == w % 2) & (rung + 1 < nt))[0]
        cu = cl + 1
        u = uniform(block(t, gid[cl], 0, seed)[..., 1])
        ca, cb = ch2[cl], ch2[cu]
        xs = energy_groups(ch2, cg, ndg, a0, b0)
        with np.errstate(invalid="ignore"):
            D = 0.5 * (beta[rung[cl]] - beta[rung[cl] + 1]) * (xs[cl] - xs[cu])
            sw = np.where(~np.isinf(ca) & ~np.isinf(cb), np.log(u) < D, np.isinf(ca) & ~np.isinf(cb))
        for name, m in zip(BRANCHES, (~np.isinf(ca) & ~np.isinf(cb), np.isinf(ca) & ~np.isinf(cb), ~np.isinf(ca) & np.isinf(cb),
                                      np.isinf(ca) & np.isinf(cb))):
            seen[name] = int(m.sum())
        l, h = cl[sw], cu[sw]
        cur[:nlay, l], cur[:nlay, h] = cur[:nlay, h].copy(), cur[:nlay, l].copy()
        ch2[l], ch2[h] = ch2[h].copy(), ch2[l].copy()
        cg[:, l], cg[:, h] = cg[:, h].copy(), cg[:, l].copy()
        np.add.at(swap_try, (cs[cl], rung[cl]), 1)
        np.add.at(swap_acc, (cs[cl], rung[cl]), sw.astype(np.int64))
    # the records: the rung-0 chains; the best model over every chain, by raw chi2
    sums, hist, accepted = st["sums"].copy(), st["hist"].copy(), st["accepted"].copy()
    best, best_chi2 = st["best"].copy(), st["best_chi2"].copy()
    nsum, ncnt = gs["nsum"].copy(), gs["ncnt"].copy()
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
        rec = cold & ~np.isinf(ch2)
        for g in range(G):   # B_g at the state of every rung-0 chain with a finite chi2, for the groups with data
            rg = rec & (ndg[g] > 0)
            B = float(np.float32(b0[g])) + 0.5 * cg[g, rg]
            nsum[0, g, rg] += np.sqrt(B)
            nsum[1, g, rg] += B
        ncnt[rec] += 1
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
    return new, ntp, cov, dict(gs, chi2g=cg, nsum=nsum, ncnt=ncnt), acc, acc_win, factored, seen


def result(gs, wdat_cells, cells, ncell, nchain, ntemp):
    """dazim_mc_noise_groups_result from the groups' record: wdat_cells [kmax][ncell] fp32 (the inner cells), cells the sampled
    inner-cell indices.  Returns dict lam_mean, lam_std [G][ncell] fp32 and ndata [G][ncell] int32"""
    G = gs["ngroup"]
    nd = ndata_groups(wdat_cells, gs["group_of_period"], G).astype(np.int32)
    lam_mean, lam_std = np.zeros((G, ncell), np.float32), np.zeros((G, ncell), np.float32)
    for g in range(G):
        a0 = float(np.float32(gs["a0"][g]))
        for cs, cell in enumerate(cells):
            if nd[g, cell] == 0:
                continue
            n, s0, s1 = 0, 0.0, 0.0
            for ch in range(0, nchain, ntemp):
                col = cs * nchain + ch
                n += int(gs["ncnt"][col])
                s0 += gs["nsum"][0, g, col]
                s1 += gs["nsum"][1, g, col]
            if n == 0:
                lam_mean[g, cell] = lam_std[g, cell] = np.nan
                continue
            a = a0 + 0.5 * int(nd[g, cell])
            lm = mc_ref.gamma_ratio(a) * s0 / float(n)
            lam_mean[g, cell] = np.float32(lm)
            lam_std[g, cell] = np.nan if a <= 1.0 else np.float32(math.sqrt(max(s1 / (float(n) * (a - 1.0)) - lm * lm, 0.0)))
    return dict(lam_mean=lam_mean, lam_std=lam_std, ndata=nd)


def sample(forward, nburn, nsample, nadapt, gcell, nchain, vmin, vmax, vlast, cobs, wdat, nbin, seed, grp, a0, b0, step0=0.05, ntemp=1,
           tmax=1.0, nswap=1, kind=0):
    """mc_ref.sample with the groups (grp [kmax], a0, b0 [G]) in place of its (a0, b0).  Returns (state, ladder, groups' state)"""
    nlay, ncs = vmin.shape
    ncol = ncs * nchain
    rep = lambda x: np.repeat(x, nchain, axis=-1)
    lo, hi = rep(vmin.astype(np.float64)), rep(vmax.astype(np.float64))
    cb, wd = rep(cobs), rep(wdat)
    _, _, _, gid = layout(ncol, nchain, ntemp, gcell)
    prop = np.concatenate([mc_ref.start_models(gid, lo, hi, seed), rep(vlast.astype(np.float32))[None]])
    st = dict(cur=prop.copy(), chi2=np.full(ncol, np.inf), scale=np.full(ncs, step0, np.float32), step=0,
              sums=np.zeros((2, nlay, ncol)), hist=np.zeros((ncs, nlay, nbin), np.uint32), accepted=np.zeros(ncol, np.int64),
              best=np.zeros((nlay, ncs), np.float32), best_chi2=np.full(ncs, np.inf))
    tp = dict(ntemp=ntemp, tmax=tmax, nswap=nswap)
    if ntemp > 1:
        tp.update(beta=mc_ref.ladder(ntemp, tmax), scale=np.full((ncs, ntemp), step0, np.float32),
                  swap_try=np.zeros((ncs, ntemp - 1), np.int64), swap_acc=np.zeros((ncs, ntemp - 1), np.int64))
    tp = mc_ref.ladder_state(st, tp)
    cov = mc_ref.empty_cov(ncs, nlay) if kind == 1 else None
    gs = empty_groups(grp, a0, b0, ncol)
    acc_win = np.zeros((ncs, ntemp), np.int64)
    nbd = 0
    for t in range(1, nburn + nsample + 1):
        record = t > nburn
        adapt = False
        if not record and t > 1:
            nbd += 1
            adapt = nbd % nadapt == 0
        pv = forward(prop)
        st, tp, cov, gs, _, acc_win, _, _ = step(st, tp, cov, gs, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cb,
                                                 wd, nbin, seed)
        prop = mc_ref.proposals(st["cur"], tp["scale"], cov, prop, t, gcell, nchain, lo, hi, seed)
    return st, tp, gs


# ---- the linear problem of the group tests, and its posterior by quadrature ---------------------------------------------------------

def linear_problem(sig=0.02, noise=(0.02, 0.06), a0=2.0, b0=1.0, half=0.06, seed=11):
    """c = K v: 16 cells, 2 knots, 2 groups x 12 periods (group 0 first), w = 1 / sig as fp32; group 0 has data noise noise[0] (the
    assumed level), group 1 noise[1] (3 x it).  The box is the least-squares model +- half."""
    rng = np.random.default_rng(seed)
    ncell, nper, nlay = 16, 12, 2
    kmax = 2 * nper
    K = np.vstack([np.eye(nlay)] * nper) + 0.35 * rng.random((kmax, nlay))
    grp = np.repeat(np.arange(2), nper).astype(np.int32)
    vtrue = rng.uniform(3.0, 4.0, (ncell, nlay))
    sd = np.where(grp == 0, noise[0], noise[1])
    cobs = (vtrue @ K.T + rng.normal(0, 1, (ncell, kmax)) * sd).astype(np.float32)
    ls = np.linalg.lstsq(K, cobs.astype(np.float64).T, rcond=None)[0].T       # [ncell][nlay]
    return dict(K=K, grp=grp, cobs=cobs, w=np.float32(1.0 / sig), vmin=(ls - half).astype(np.float32),
                vmax=(ls + half).astype(np.float32), ncell=ncell, kmax=kmax, nlay=nlay, a0=np.full(2, a0, np.float32),
                b0=np.full(2, b0, np.float32))


def quadrature(pb, n):
    """the posterior moments of the linear problem on an n x n midpoint grid over the box itself (the truncation is exact): posterior
    proportional to prod_g B_g(v)^-a_g; E[lambda_g] = g(a_g) E[sqrt(B_g)], E[lambda_g^2] = E[B_g] / (a_g - 1).  fp64.
    Returns dict mu, sd [ncell][nlay], lam_mean, lam_std [G][ncell]"""
    K, grp, ncell, nlay = pb["K"], pb["grp"], pb["ncell"], pb["nlay"]
    G = len(pb["a0"])
    w = float(pb["w"])
    mu, sd = np.zeros((ncell, nlay)), np.zeros((ncell, nlay))
    lam1, lam2 = np.zeros((G, ncell)), np.zeros((G, ncell))
    for c in range(ncell):
        lo, hi = pb["vmin"][c].astype(np.float64), pb["vmax"][c].astype(np.float64)
        ax = [lo[k] + (np.arange(n) + 0.5) * (hi[k] - lo[k]) / n for k in range(nlay)]
        V = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, nlay)
        r = w * (pb["cobs"][c].astype(np.float64)[None, :] - V @ K.T)
        B, a, logp = [], [], np.zeros(len(V))
        for g in range(G):
            sel = grp == g
            a.append(float(pb["a0"][g]) + 0.5 * sel.sum())
            B.append(float(pb["b0"][g]) + 0.5 * (r[:, sel] ** 2).sum(axis=1))
            logp -= a[g] * np.log(B[g])
        p = np.exp(logp - logp.max())
        p /= p.sum()
        mu[c] = p @ V
        sd[c] = np.sqrt(p @ (V - mu[c]) ** 2)
        for g in range(G):
            lam1[g, c] = mc_ref.gamma_ratio(a[g]) * (p @ np.sqrt(B[g]))
            lam2[g, c] = (p @ B[g]) / (a[g] - 1.0)
    return dict(mu=mu, sd=sd, lam_mean=lam1, lam_std=np.sqrt(lam2 - lam1 ** 2))


def reference(pb, n0=128, tol=1e-4):
    """quadrature refined (n doubled) until every moment moves by less than tol relative; returns (moments, n, the last move)"""
    prev, n = quadrature(pb, n0), n0
    while True:
        n *= 2
        cur = quadrature(pb, n)
        move = max(np.abs(cur[k] / prev[k] - 1).max() for k in ("mu", "sd", "lam_mean", "lam_std"))
        if move < tol:
            return cur, n, move
        prev = cur
