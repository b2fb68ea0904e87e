"""NumPy restatement of the noise scales of the Monte-Carlo step, one per group of periods (dazim_mc_set_noise_groups and, as one
group, dazim_mc_set_noise; include/dazim.h): chi2_g beside chi2, the energy X = sum_g 2 a_g log(b0_g + chi2_g /
2), the record per group and its result, as tests/mc_ref.py's step and sample use them; and the linear problem of the group tests."""
import math

import numpy as np

MAXGRP = 4


def gamma_ratio(a):
    """g(a) = Gamma(a - 1/2) / Gamma(a) as the library's table forms it"""
    return math.exp(math.lgamma(a - 0.5) - math.lgamma(a))


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
            lm = gamma_ratio(a) * s0 / float(n)
            lam_mean[g, cell] = np.float32(lm)
            lam_std[g, cell] = np.nan if a <= 1.0 else np.float32(math.sqrt(max(s1 / (float(n) * (a - 1.0)) - lm * lm, 0.0)))
    return dict(lam_mean=lam_mean, lam_std=lam_std, ndata=nd)


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
            lam1[g, c] = gamma_ratio(a[g]) * (p @ np.sqrt(B[g]))
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
