"""NumPy restatement of the radial mode of dazim_mc (dazim_mc_set_radial, include/dazim.h): the handle's
knots are the stacked vector [Vsv_0..Vsv_{n-1}, Vsh_0..Vsh_{n-1}, deepest].  The step itself is tests/mc_ref.py's on 2n knots; here
are the radial Q (which a test puts in place of mc_ref's and mc_step_check's `prior_q`, patched()), the split of the proposals into
the two models of the forward calls, the record of xi = (Vsh / Vsv)^2, the Voigt average and Vsv Vsh, the final statistics, and a
CPU `sample`.  Every operation is the library's in the same order and precision; only sqrt may differ in the last bit."""
import contextlib

import numpy as np

from tests import mc_ref, mc_step_check


def radial_q(v, vref, smooth, damp, couple):
    """Q of the columns of the stacked knots v [2n][ncol] fp32 about vref [2n][ncol] fp32 in the library's order: q1 and q2 run on
    through the Vsv and then the Vsh profile in knot order, L's rule inside each profile; qc = sum (vh_a - vv_a)^2 in knot order;
    Q = (s2 q1 + d2 q2) + m2 qc with s2, d2, m2 the squares in fp64 of the fp32 smooth, damp and couple"""
    s2 = float(np.float32(smooth)) * float(np.float32(smooth))
    d2 = float(np.float32(damp)) * float(np.float32(damp))
    m2 = float(np.float32(couple)) * float(np.float32(couple))
    n = v.shape[0] // 2
    assert v.shape[0] == 2 * n
    v64 = v.astype(np.float64)
    q1, q2, qc = np.zeros(v.shape[1]), np.zeros(v.shape[1]), np.zeros(v.shape[1])
    for k0 in (0, n):
        d = v64[k0:k0 + n] - vref[k0:k0 + n].astype(np.float64)
        for a in range(n):
            t = 2.0 * d[a] if a in (0, n - 1) else (2.0 * d[a] - d[a - 1]) - d[a + 1]
            q1 = q1 + t * t
            q2 = q2 + d[a] * d[a]
    for a in range(n):
        c = v64[n + a] - v64[a]
        qc = qc + c * c
    return (s2 * q1 + d2 * q2) + m2 * qc


def prior_q_of(couple):
    """the radial Q under the signature of tests/mc_prior_ref.prior_q"""
    return lambda v, vref, smooth, damp: radial_q(v, vref, smooth, damp, couple)


@contextlib.contextmanager
def patched(couple):
    """mc_ref.step and mc_step_check.drive reach Q through the name prior_q in their own namespaces: the radial Q there, for as long
    as the block runs (a test does the same with pytest's monkeypatch)"""
    q = prior_q_of(couple)
    old = mc_ref.prior_q, mc_step_check.prior_q
    mc_ref.prior_q = mc_step_check.prior_q = q
    try:
        yield q
    finally:
        mc_ref.prior_q, mc_step_check.prior_q = old


def precision(n, smooth, damp, couple):
    """P2 = [[P + m2 I, -m2 I], [-m2 I, P + m2 I]], P = s2 L^T L + d2 I, built densely (dazim_column_resolution_radial's)"""
    L = 2.0 * np.eye(n)
    for i in range(1, n - 1):
        L[i, i - 1] = L[i, i + 1] = -1.0
    P = smooth ** 2 * L.T @ L + damp ** 2 * np.eye(n)
    m2 = couple ** 2 * np.eye(n)
    return np.block([[P + m2, -m2], [-m2, P + m2]])


def split(prop):
    """the two models of the forward calls from the proposals prop [2n+1][ncol]: (vsv, vsh), each [n+1][ncol]; vsh is rows n..2n as
    they lie, vsv the Vsv knots beside the deepest row"""
    n = (prop.shape[0] - 1) // 2
    return np.concatenate([prop[:n], prop[2 * n:]]), prop[n:].copy()


def xi_range(lo, hi):
    """the exact range of xi per knot pair from the boxes lo, hi [2n][..] (fp64 of the fp32 bounds): ((lo_h / hi_v)^2, (hi_h / lo_v)^2)"""
    n = lo.shape[0] // 2
    rl, rh = lo[n:] / hi[:n], hi[n:] / lo[:n]
    return rl * rl, rh * rh


def empty_record(n, ncol, ncs, nbin, couple=0.0):
    return dict(n=n, couple=float(np.float32(couple)), rsum=np.zeros((5, n, ncol)), ngt1=np.zeros((n, ncol), np.int64),
                xhist=np.zeros((ncs, n, nbin), np.uint32))


def record(rs, cur, cold, cs, lo, hi, nbin):
    """the radial record of one recorded step: cur [2n+1][ncol] the states after the decision and any swap, cold [ncol] the rung-0
    columns, cs [ncol] the sampled cell of every column, lo, hi [2n][ncol] fp64.  Returns the new record."""
    n = rs["n"]
    rsum, ngt1, xhist = rs["rsum"].copy(), rs["ngt1"].copy(), rs["xhist"].copy()
    vv, vh = cur[:n, cold].astype(np.float64), cur[n:2 * n, cold].astype(np.float64)
    r = vh / vv
    xi = r * r
    V = np.sqrt((2.0 * vv * vv + vh * vh) / 3.0)
    for e, t in enumerate((xi, xi * xi, vv * vh, V, V * V)):
        rsum[e][:, cold] += t
    ngt1[:, cold] += xi > 1.0
    xlo, xhi = xi_range(lo[:, cold], hi[:, cold])
    b = np.clip(((xi - xlo) / (xhi - xlo) * float(nbin)).astype(np.int64), 0, nbin - 1)
    for a in range(n):
        np.add.at(xhist, (cs[cold], a, b[a]), 1)
    return dict(rs, rsum=rsum, ngt1=ngt1, xhist=xhist)


def final(st, rs, vmin, vmax, vel0_knots, cells, ncell, nchain, ntemp, nrec, nbin):
    """k_mc_radial_final from a state `st` and a radial record `rs`, over the rung-0 chains in chain order: vmin, vmax, vel0_knots
    [2n][ncell] fp32 (the inner cells), cells the sampled inner-cell indices.  Returns dict xi_mean, xi_std, xi_rhat, p_gt1, corr_vh,
    voigt_mean, voigt_std [n][ncell] and xi_q [3][n][ncell] as the library forms them (fp32)."""
    n = rs["n"]
    nlay = 2 * n
    v0 = vel0_knots.astype(np.float64)
    r0 = v0[n:nlay] / v0[:n]
    xi0 = (r0 * r0).astype(np.float32)
    V0 = np.sqrt((2.0 * v0[:n] * v0[:n] + v0[n:nlay] * v0[n:nlay]) / 3.0).astype(np.float32)
    nan = lambda: np.full((n, ncell), np.nan, np.float32)
    out = dict(xi_mean=xi0.copy(), xi_std=np.zeros((n, ncell), np.float32), xi_q=np.stack([xi0] * 3), xi_rhat=nan(), p_gt1=nan(),
               corr_vh=nan(), voigt_mean=V0.copy(), voigt_std=np.zeros((n, ncell), np.float32))
    ncold = nchain // ntemp
    N, Mc = float(nrec), float(ncold)
    tot = N * Mc
    lo64, hi64 = vmin.astype(np.float64), vmax.astype(np.float64)
    xlo, xhi = xi_range(lo64, hi64)
    for cs, cell in enumerate(cells):
        cols = cs * nchain + np.arange(0, nchain, ntemp)
        for a in range(n):
            s1 = s2 = sm = sv = svv = sh = shh = svh = g1 = g2 = 0.0
            gt = 0
            for col in cols:
                x1 = rs["rsum"][0, a, col]
                s1 += x1
                s2 += rs["rsum"][1, a, col]
                sm += x1 / N
                svh += rs["rsum"][2, a, col]
                g1 += rs["rsum"][3, a, col]
                g2 += rs["rsum"][4, a, col]
                gt += int(rs["ngt1"][a, col])
                sv += st["sums"][0, a, col]
                svv += st["sums"][1, a, col]
                sh += st["sums"][0, n + a, col]
                shh += st["sums"][1, n + a, col]
            mu = s1 / tot
            out["xi_mean"][a, cell] = np.float32(mu)
            out["xi_std"][a, cell] = np.float32(np.sqrt(max(s2 / tot - mu * mu, 0.0)))
            if ncold > 1 and nrec > 1:
                W = B = 0.0
                mbar = sm / Mc
                for col in cols:
                    x1, x2 = rs["rsum"][0, a, col], rs["rsum"][1, a, col]
                    mj = x1 / N
                    W += (x2 - N * mj * mj) / (N - 1.0)
                    B += (mj - mbar) * (mj - mbar)
                W /= Mc
                B *= N / (Mc - 1.0)
                if W > 0.0:
                    out["xi_rhat"][a, cell] = np.float32(np.sqrt(((N - 1.0) / N * W + B / N) / W))
            h = rs["xhist"][cs, a].astype(np.float64)
            lo, hi = float(xlo[a, cell]), float(xhi[a, cell])
            for e, qv in enumerate((0.025, 0.5, 0.975)):
                target, cum, pos = qv * tot, 0.0, float(nbin)
                for b in range(nbin):
                    if h[b] > 0.0 and cum + h[b] >= target:
                        pos = b + (target - cum) / h[b]
                        break
                    cum += h[b]
                out["xi_q"][e, a, cell] = np.float32(lo + pos * (hi - lo) / nbin)
            out["p_gt1"][a, cell] = np.float32(float(gt) / tot)
            ev, eh = sv / tot, sh / tot
            dv, dh = np.sqrt(max(svv / tot - ev * ev, 0.0)), np.sqrt(max(shh / tot - eh * eh, 0.0))
            if dv > 0.0 and dh > 0.0:
                out["corr_vh"][a, cell] = np.float32((svh / tot - ev * eh) / (dv * dh))
            gm = g1 / tot
            out["voigt_mean"][a, cell] = np.float32(gm)
            out["voigt_std"][a, cell] = np.float32(np.sqrt(max(g2 / tot - gm * gm, 0.0)))
    return out


def sample(forward_v, forward_h, nburn, nsample, nadapt, gcell, nchain, vmin, vmax, vlast, cobs, wdat, nbin, seed, couple, prior=None,
           **modes):
    """the whole radial sampler from the restatements alone: mc_ref.sample on the stacked knots with the radial Q in place, the
    curves of a proposal being forward_v(vsv [n+1][ncol]) (rows [0, kR)) above forward_h(vsh [n+1][ncol]), and the radial record of
    every recorded step.  vmin, vmax [2n][ncs], vlast [ncs], cobs, wdat [kmax][ncs]; prior: None or (smooth, damp, vref [2n][ncs]); a
    couple > 0 alone puts the prior on about vmin (whose terms then carry the factor 0).  modes: mc_ref.sample's other keywords.
    Returns (state, ladder, noise record or None, radial record)."""
    nlay, ncs = vmin.shape
    n, ncol, ntemp = nlay // 2, ncs * nchain, modes.get("ntemp", 1)
    rep = lambda x: np.repeat(x, nchain, axis=-1)
    lo, hi = rep(vmin.astype(np.float64)), rep(vmax.astype(np.float64))
    _, cs, rung, _ = mc_ref.layout(ncol, nchain, ntemp, gcell)
    box = dict(rs=empty_record(n, ncol, ncs, nbin, couple))
    if prior is None and couple != 0:
        prior = (0.0, 0.0, vmin)

    def forward(prop):
        vsv, vsh = split(prop)
        return np.concatenate([forward_v(vsv), forward_h(vsh)])

    def each(t, r):
        if t > nburn:
            box["rs"] = record(box["rs"], r["st"]["cur"], rung == 0, cs, lo, hi, nbin)

    with patched(couple):
        # (mc_ref.sample's start record comes from mc_prior_ref.empty_prior, whose Q is its own module's: the same patch there)
        from tests import mc_prior_ref
        old = mc_prior_ref.prior_q
        mc_prior_ref.prior_q = prior_q_of(couple)
        try:
            st, tp, ns = mc_ref.sample(forward, nburn, nsample, nadapt, gcell, nchain, vmin, vmax, vlast, cobs, wdat, nbin, seed,
                                       prior=prior, each=each, **modes)
        finally:
            mc_prior_ref.prior_q = old
    return st, tp, ns, box["rs"]


def linear_problem(seed=9):
    """the linear-Gaussian problem of the radial tests: 16 cells, n = 2, c_R = K_R vv (6 periods) and c_L = K_L vh (6 periods),
    sigma 0.02 (w = 1 / sigma as fp32), the prior smooth 20, damp 20 about 3.5 and couple 40 (std 0.025 km/s of Vsh - Vsv): data
    and prior weigh alike.  The posterior of the stacked knots is the Gaussian of precision A = K^T W^2 K + P2 (precision()) with
    mean A^-1 (K^T W^2 c + Pb vref), Pb = P2 without the coupling; the box is mean +- 5 sd.  xi's mean and std and P(xi > 1) per
    cell and knot pair come from 80 x 80 Gauss-Hermite quadrature of the pair's bivariate Gaussian in fp64."""
    rng = np.random.default_rng(seed)
    ncell, n, kr, kl, sig, smooth, damp, couple = 16, 2, 6, 6, 0.02, 20.0, 20.0, 40.0
    KR = np.vstack([np.eye(n)] * 3) + 0.35 * rng.random((kr, n))
    KL = np.vstack([np.eye(n)] * 3) + 0.35 * rng.random((kl, n))
    K = np.block([[KR, np.zeros((kr, n))], [np.zeros((kl, n)), KL]])
    vv = rng.uniform(3.3, 3.7, (ncell, n))
    vtrue = np.concatenate([vv, vv * rng.uniform(0.98, 1.04, (ncell, n))], axis=1)
    cobs = (vtrue @ K.T + rng.normal(0, sig, (ncell, kr + kl))).astype(np.float32)
    w32 = float(np.float32(1.0 / sig))
    vref = np.full(2 * n, 3.5)
    cov = np.linalg.inv(K.T @ K * w32 ** 2 + precision(n, smooth, damp, couple))
    mu = (cobs.astype(np.float64) @ K * w32 ** 2 + precision(n, smooth, damp, 0.0) @ vref) @ cov      # [ncell][2n]
    sd = np.sqrt(np.diag(cov))
    corr = np.array([cov[a, n + a] / (sd[a] * sd[n + a]) for a in range(n)])
    x, w = np.polynomial.hermite_e.hermegauss(80)
    w = w / w.sum()
    xi_mean, xi_std, p_gt1 = (np.zeros((ncell, n)) for _ in range(3))
    for a in range(n):
        Lc = np.linalg.cholesky(cov[np.ix_([a, n + a], [a, n + a])])
        z = np.stack(np.meshgrid(x, x, indexing="ij"))                  # [2][80][80]
        ww = w[:, None] * w[None, :]
        for c in range(ncell):
            v = mu[c, [a, n + a]][:, None, None] + np.tensordot(Lc, z, 1)
            xi = (v[1] / v[0]) ** 2
            m1 = (ww * xi).sum()
            xi_mean[c, a], xi_std[c, a] = m1, np.sqrt((ww * xi * xi).sum() - m1 * m1)
            # P(vh > vv) of a Gaussian difference, exactly (vv > 0 on all of the box)
            s = np.sqrt(cov[a, a] + cov[n + a, n + a] - 2.0 * cov[a, n + a])
            from math import erf
            p_gt1[c, a] = 0.5 * (1.0 + erf((mu[c, n + a] - mu[c, a]) / (s * np.sqrt(2.0))))
    return dict(ncell=ncell, n=n, kr=kr, kl=kl, sig=sig, smooth=smooth, damp=damp, couple=couple, KR=KR, KL=KL, cobs=cobs, mu=mu, sd=sd,
                corr=corr, xi_mean=xi_mean, xi_std=xi_std, p_gt1=p_gt1, vmin=(mu - 5.0 * sd).astype(np.float32),
                vmax=(mu + 5.0 * sd).astype(np.float32), w=np.float32(1.0 / sig), vref=vref)


def linear_figures(pb, mean, std, corr, xi_mean, xi_std, p_gt1):
    """what the linear tests hold against the analytic posterior, each the maximum over cells and knots: mean, std [ncell][2n];
    corr, xi_mean, xi_std, p_gt1 [ncell][n].  dict mean_sd (|mean - mu| / sd), std_ratio (|std / sd - 1|), corr (|corr - analytic|),
    xi_mean_sd (|xi_mean - quadrature| / quadrature's std), xi_std_ratio, p_gt1 (|p - analytic|)"""
    return dict(mean_sd=(np.abs(mean - pb["mu"]) / pb["sd"]).max(), std_ratio=np.abs(std / pb["sd"] - 1).max(), corr=np.abs(corr - pb["corr"]).max(),
                xi_mean_sd=(np.abs(xi_mean - pb["xi_mean"]) / pb["xi_std"]).max(), xi_std_ratio=np.abs(xi_std / pb["xi_std"] - 1).max(),
                p_gt1=np.abs(p_gt1 - pb["p_gt1"]).max())


# the bars of the linear tests: twice the figures of the restatement's own run (tests/test_mc_radial_ref_cpu.py measures them: 0.0308,
# 0.0168, 0.0217, 0.0261, 0.0155, 0.0063), rounded up to two digits
LINEAR_BARS = dict(mean_sd=0.062, std_ratio=0.034, corr=0.044, xi_mean_sd=0.053, xi_std_ratio=0.031, p_gt1=0.013)
LINEAR_STEPS = (1500, 4000)
