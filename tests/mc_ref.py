"""NumPy restatement of the Monte-Carlo step of dazim_mc (include/dazim.h): Philox4x32-10, the draws, and one
step from a copy of the handle's state, in every mode: proposal kind 0 or 1 (the covariance sums, the factor at the adaptation
points, y = L z), a ladder of rungs or none (the decision at rung r, the scale per rung, the swaps, the records of the rung-0 chains),
the fixed noise level or noise scales integrated out (every scale a group of periods, tests/mc_groups_ref.py: the energy X = sum_g
2 a_g log(b0_g + chi2_g / 2) wherever a decision is taken, the noise record and its result), the Gaussian prior or none (X + Q in
place of X, tests/mc_prior_ref.py).  An untempered handle is a ladder of one rung with beta = 1, which leaves every product
unchanged.  Every operation is the library's in the same order and precision (the library is compiled without FMA contraction); only
log, sqrt, cos and sin may differ in the last bit, and lgamma and exp of the noise result's table in the last few."""
import numpy as np

from tests import mc_groups_ref
from tests.mc_groups_ref import chi2_groups, empty_groups, energy_groups, gamma_ratio, ndata_groups  # noqa: F401
from tests.mc_prior_ref import empty_prior, prior_q

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
TWO_PI = 6.283185307179586
MAXFOLD = 8     # reflections of a proposal into its box (4 always suffice for a step scale <= 0.5)
COV_MIN = 8     # kind 1: states per knot before a window factors
RIDGE = 1e-8
BRANCHES = ("both_finite", "lower_inf", "upper_inf", "both_inf")


def philox4x32_10(ctr, key):
    """ctr: uint32 array [..., 4], key: uint32 array [..., 2] (broadcast) -> uint32 [..., 4]"""
    c = [np.asarray(ctr[..., i], np.uint32).copy() for i in range(4)]
    k0 = np.asarray(key[..., 0], np.uint32).copy()
    k1 = np.asarray(key[..., 1], np.uint32).copy()
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0 = (k0 + W0).astype(np.uint32)
                k1 = (k1 + W1).astype(np.uint32)
            p0 = M0 * c[0].astype(np.uint64)
            p1 = M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, axis=-1)


def block(step, gid, blk, seed):
    """the four words of Philox with counter (step, gid, blk, 0) and key (seed low, seed high); gid an array"""
    gid = np.asarray(gid, np.uint32)
    ctr = np.zeros(gid.shape + (4,), np.uint32)
    ctr[..., 0] = np.uint32(step & 0xFFFFFFFF)
    ctr[..., 1] = gid
    ctr[..., 2] = np.uint32(blk)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
    return philox4x32_10(ctr, key)


def uniform(w):
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def normals(step, gid, nlay, seed):
    """z [nlay][len(gid)] of step `step`"""
    out = []
    for q in range((nlay + 3) // 4):
        w = block(step, gid, 1 + q, seed)
        r0 = np.sqrt(-2.0 * np.log(uniform(w[..., 0])))
        a0 = TWO_PI * uniform(w[..., 1])
        r1 = np.sqrt(-2.0 * np.log(uniform(w[..., 2])))
        a1 = TWO_PI * uniform(w[..., 3])
        out += [r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)]
    return np.array(out[:nlay])


def start_models(gid, lo, hi, seed):
    """the prior draws of step 0: lo, hi [nlay][len(gid)] fp64 -> fp32"""
    nlay = lo.shape[0]
    out = np.zeros(lo.shape, np.float32)
    for q in range((nlay + 3) // 4):
        w = block(0, gid, 1 + q, seed)
        for e in range(4):
            k = 4 * q + e
            if k < nlay:
                out[k] = (lo[k] + (hi[k] - lo[k]) * uniform(w[..., e])).astype(np.float32)
    return out


def chi2(pv, cobs, wdat):
    """pv [kmax][ncol] fp64, cobs / wdat [kmax][ncol] fp32 (the column's cell's values) -> chi2 [ncol], in period order"""
    kmax, ncol = pv.shape
    s = np.zeros(ncol, np.float64)
    for p in range(kmax):
        w = wdat[p].astype(np.float64)
        r = w * (cobs[p].astype(np.float64) - pv[p])
        data = wdat[p] != 0
        s = np.where(data, np.where(pv[p] == 0.0, np.inf, s + r * r), s)
    return s


def pairs(nlay):
    """rows a and columns c of the packed lower triangle: pair (a, c), c <= a, at a (a + 1) / 2 + c"""
    a = np.array([i for i in range(nlay) for _ in range(i + 1)])
    c = np.array([j for i in range(nlay) for j in range(i + 1)])
    return a, c


def empty_cov(ncs, nlay):
    npair = nlay * (nlay + 1) // 2
    return dict(kind=1, cov_n=np.zeros(ncs, np.int64), cov_s1=np.zeros((ncs, nlay)), cov_s2=np.zeros((ncs, npair)),
                chol=np.zeros((ncs, npair)), cov_set=np.zeros(ncs, np.int32))


def covariance(n, s1, s2, nlay):
    """the full symmetric matrix the factor starts from"""
    a, c = pairs(nlay)
    dn = float(n)
    m = s1 / dn
    cp = s2 / dn - m[a] * m[c]
    cp[a == c] += RIDGE
    C = np.zeros((nlay, nlay))
    C[a, c] = cp
    C[c, a] = cp
    return C


def cholesky(C):
    """right-looking, column by column, one update per element per column; returns (ok, packed factor)"""
    n = C.shape[0]
    L = np.tril(C)
    for c in range(n):
        p = L[c, c]
        if not (np.isfinite(p) and p > 0.0):
            return False, None
        d = np.sqrt(p)
        L[c + 1:, c] = L[c + 1:, c] / d
        L[c, c] = d
        col = L[c + 1:, c]
        L[c + 1:, c + 1:] -= np.tril(col[:, None] * col[None, :])
    a, cc = pairs(n)
    return True, L[a, cc]


def ladder(ntemp, tmax):
    """beta_r = tmax^(-r / (ntemp - 1)), beta_0 = 1"""
    return np.array([1.0] + [float(tmax) ** (-r / (ntemp - 1)) for r in range(1, ntemp)])


def layout(ncol, nchain, ntemp, gcell):
    ncs = ncol // nchain
    cs = np.repeat(np.arange(ncs), nchain)
    ch = np.tile(np.arange(nchain), ncs)
    gid = (gcell[cs] * nchain + ch).astype(np.uint32)
    return ncs, cs, ch % ntemp, gid


def ladder_state(st, tp):
    """the ladder of a handle as step() takes it; an untempered handle (temper_state() without arrays) is one rung at beta 1"""
    if tp["ntemp"] > 1:
        return tp
    ncs = st["scale"].size
    return dict(tp, beta=np.array([1.0]), scale=st["scale"].reshape(ncs, 1).copy(), swap_try=np.zeros((ncs, 0), np.int64),
                swap_acc=np.zeros((ncs, 0), np.int64))


def ndata(wdat):
    """periods with data per column (wdat [kmax][ncol]) or per cell (wdat [kmax][ncell])"""
    return (wdat != 0).sum(axis=0)


def energy(chi2, a, b0):
    """X = 2 a log(B(chi2)), B = (double)b0 + chi2 / 2; +inf at chi2 = +inf"""
    with np.errstate(invalid="ignore"):
        return 2.0 * a * np.log(float(np.float32(b0)) + 0.5 * chi2)


def empty_noise(a0, b0, ncol):
    return dict(a0=float(np.float32(a0)), b0=float(np.float32(b0)), nsum=np.zeros((2, ncol)), ncnt=np.zeros(ncol, np.int64))


def as_groups(ns, chi2, kmax):
    """the noise record in the groups' form: None (the fixed level) and a groups record (noise_groups_state(), empty_groups()) as they
    are; the single-scale record (noise_state(), empty_noise()) as its one group of every period, whose chi2_g is chi2 itself"""
    if ns is None or "ngroup" in ns:
        return ns
    return dict(ngroup=1, group_of_period=np.zeros(kmax, np.int32), a0=np.float32([ns["a0"]]), b0=np.float32([ns["b0"]]),
                chi2g=None if chi2 is None else chi2[None], nsum=ns["nsum"][:, None], ncnt=ns["ncnt"])


def step(st, tp, cov, ns, pr, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cobs, wdat, nbin, seed):
    """one step from the state `st` (MonteCarlo.state()), the ladder `tp` (ladder_state(): one rung = untempered), `cov`
    (MonteCarlo.cov_state() for kind 1, None for kind 0), the noise record `ns` (None for the fixed noise level: the energy is chi2
    itself; MonteCarlo.noise_state() or empty_noise(); MonteCarlo.noise_groups_state() or empty_groups(): every scale is a group,
    as_groups()), the prior record `pr` (empty_prior(), or MonteCarlo.prior_state() with vref per column; None: off) and the
    proposals prop [nz][ncol]; gcell [ncs] the inner-cell index of each sampled cell; lo, hi [nlay][ncol] fp64 and cobs, wdat
    [kmax][ncol] per column; acc_win [ncs][ntemp] the burn-in window counts.
    Returns a dict: st, tp, cov (with the restated factor, or None), ns (in the form it came in, or None), pr (or None), acc (the
    decisions [ncol]), acc_win, factored ({cs: C} of the cells factored in this step), seen ({branch: pairs} of the swap rule's four
    cases) and diff ({"dec", "swap"}: decisions and swap rules that the prior made other than the energies alone would have).  The
    next proposals come from proposals(), so that a test can form them from the library's factor."""
    nz, ncol = prop.shape
    nlay = nz - 1
    nt, nswap, beta = tp["ntemp"], tp["nswap"], tp["beta"]
    ncold = nchain // nt
    ncs, cs, rung, gid = layout(ncol, nchain, nt, gcell)
    gs = as_groups(ns, st["chi2"], pv.shape[0])
    if gs is None:
        chi2p, cgp, cg = chi2(pv, cobs, wdat), None, None
        X = lambda c2, g: c2
    else:
        G = gs["ngroup"]
        ndg = ndata_groups(wdat, gs["group_of_period"], G)
        chi2p, cgp = chi2_groups(pv, cobs, wdat, gs["group_of_period"], G)
        X = lambda c2, g: energy_groups(c2, g, ndg, gs["a0"], gs["b0"])
    qp = prior_q(prop[:nlay], pr["vref"], pr["smooth"], pr["damp"]) if pr is not None else None
    total = (lambda x, q: x + q) if pr is not None else (lambda x, q: x)
    diff = dict(dec=0, swap=0)
    first = t == 1
    if first:
        acc = np.ones(ncol, bool)
    else:
        c = st["chi2"]
        u = uniform(block(t, gid, 0, seed)[..., 0])
        xp, xc = X(chi2p, cgp), X(c, gs["chi2g"] if gs else None)
        with np.errstate(invalid="ignore"):
            rule = lambda d: np.where(np.isinf(c), ~np.isinf(chi2p), np.log(u) < -0.5 * beta[rung] * d)
            acc = rule(total(xp, qp) - total(xc, pr["q"] if pr else None))
            diff["dec"] = int((acc != rule(xp - xc)).sum())
    cur = st["cur"].copy()
    cur[:nlay, acc] = prop[:nlay, acc]
    ch2 = np.where(acc, chi2p, st["chi2"])
    if gs is not None:
        cg = np.where(acc[None, :], cgp, gs["chi2g"])
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
    # the swap round, on the totals of the states; chi2, the chi2_g and Q change columns with the knots
    swap_try, swap_acc = tp["swap_try"].copy(), tp["swap_acc"].copy()
    seen = dict.fromkeys(BRANCHES, 0)
    if nt > 1 and not first and t % nswap == 0:
        w = t // nswap
        cl = np.nonzero((rung % 2 == w % 2) & (rung + 1 < nt))[0]
        cu = cl + 1
        u = uniform(block(t, gid[cl], 0, seed)[..., 1])
        ca, cb = ch2[cl], ch2[cu]
        both = ~np.isinf(ca) & ~np.isinf(cb)
        xs = X(ch2, cg)
        with np.errstate(invalid="ignore"):
            rule = lambda d: np.where(both, np.log(u) < 0.5 * (beta[rung[cl]] - beta[rung[cl] + 1]) * d, np.isinf(ca) & ~np.isinf(cb))
            sw = rule(total(xs[cl], q[cl] if pr else None) - total(xs[cu], q[cu] if pr else None))
            diff["swap"] = int((sw != rule(xs[cl] - xs[cu])).sum())
        for name, m in zip(BRANCHES, (both, np.isinf(ca) & ~np.isinf(cb), ~np.isinf(ca) & np.isinf(cb), np.isinf(ca) & np.isinf(cb))):
            seen[name] = int(m.sum())
        l, h = cl[sw], cu[sw]
        for v in (cur[:nlay], ch2, cg, q):
            if v is not None:
                v[..., l], v[..., h] = v[..., h].copy(), v[..., l].copy()
        np.add.at(swap_try, (cs[cl], rung[cl]), 1)
        np.add.at(swap_acc, (cs[cl], rung[cl]), sw.astype(np.int64))
    # the records: the rung-0 chains; the best model over every chain, by raw chi2
    sums, hist, accepted = st["sums"].copy(), st["hist"].copy(), st["accepted"].copy()
    best, best_chi2 = st["best"].copy(), st["best_chi2"].copy()
    cold = rung == 0
    if gs is not None:
        nsum, ncnt = gs["nsum"].copy(), gs["ncnt"].copy()
    if record:
        if not first:
            accepted += acc & cold
        # the lowest chi2 of the step per cell, the first chain on ties; it replaces the best only when strictly lower
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
        if gs is not None:   # the noise record: B_g at the state of every rung-0 chain with a finite chi2, for the groups with data
            rec = cold & ~np.isinf(ch2)
            for g in range(G):
                rg = rec & (ndg[g] > 0)
                B = float(np.float32(gs["b0"][g])) + 0.5 * cg[g, rg]
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
                        if set0[e] == 0:   # the first factor: the scale of every rung restarts for the new metric
                            cov["cov_set"][e] = 1
                            scale[e, :] = np.float32(1.0) / root
                    cov["cov_n"][e] = 0
                    cov["cov_s1"][e] = 0.0
                    cov["cov_s2"][e] = 0.0
    new = dict(cur=cur, chi2=ch2, scale=scale[:, 0].copy(), step=t, sums=sums, hist=hist, accepted=accepted, best=best, best_chi2=best_chi2)
    if ns is not None:   # back in the form it came in
        ns = dict(ns, chi2g=cg, nsum=nsum, ncnt=ncnt) if "ngroup" in ns else dict(ns, nsum=nsum[:, 0], ncnt=ncnt)
    return dict(st=new, tp=dict(tp, scale=scale, swap_try=swap_try, swap_acc=swap_acc), cov=cov, ns=ns,
                pr=dict(pr, q=q) if pr is not None else None, acc=acc, acc_win=acc_win, factored=factored, seen=seen, diff=diff)


def proposals(cur, tscale, cov, prop, t, gcell, nchain, lo, hi, seed):
    """the proposals after step t from the state cur [nz][ncol], the scales tscale [ncs][ntemp] and, for kind 1, cov's packed factors
    chol [ncs][npair] and cov_set (None for kind 0): v' = v + s (hi - lo) y, y = L z where the cell has a factor, else z"""
    nz, ncol = prop.shape
    nlay = nz - 1
    ncs, cs, rung, gid = layout(ncol, nchain, tscale.shape[1], gcell)
    z = normals(t, gid, nlay, seed)
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
    for _ in range(MAXFOLD):
        below, above = v < lo, v > hi
        if not (below | above).any():
            break
        v = np.where(below, 2.0 * lo - v, np.where(above, 2.0 * hi - v, v))
    nxt = prop.copy()
    nxt[:nlay] = np.minimum(np.maximum(v, lo), hi).astype(np.float32)
    return nxt


def final(st, vmin, vmax, vel0_knots, cells, ncell, nchain, ntemp, nrec, ndec, nbin):
    """k_mc_final from a state, over the rung-0 chains (ntemp = 1: every chain): vmin, vmax, vel0_knots [nlay][ncell] fp32 (the inner
    cells), cells the sampled inner-cell indices.  Returns dict mean, std, q [3][nlay][ncell], best, rhat, accept, chi2_best as the
    library forms them (fp32).  One cold chain is taken twice, which scales every sum, count and total by an exact 2 and so leaves
    the quotients' bits alone, and R-hat is NaN."""
    nlay = vmin.shape[0]
    out = dict(mean=vel0_knots.copy(), std=np.zeros((nlay, ncell), np.float32), q=np.stack([vel0_knots] * 3), best=vel0_knots.copy(),
               rhat=np.full((nlay, ncell), np.nan, np.float32), accept=np.zeros(ncell, np.float32),
               chi2_best=np.zeros(ncell, np.float32))
    ncold = nchain // ntemp
    rep = 2 if ncold == 1 else 1
    N, Mc = float(nrec), float(ncold * rep)
    for cs, cell in enumerate(cells):
        cols = np.repeat(cs * nchain + np.arange(0, nchain, ntemp), rep)
        for k in range(nlay):
            s1 = s2 = sm = 0.0
            for col in cols:
                a, b = st["sums"][0, k, col], st["sums"][1, k, col]
                s1 += a
                s2 += b
                sm += a / N
            mu = s1 / (N * Mc)
            out["mean"][k, cell] = np.float32(mu)
            out["std"][k, cell] = np.float32(np.sqrt(max(s2 / (N * Mc) - mu * mu, 0.0)))
            W = B = 0.0
            mbar = sm / Mc
            for col in cols:
                a, b = st["sums"][0, k, col], st["sums"][1, k, col]
                mj = a / N
                W += (b - N * mj * mj) / (N - 1.0)
                B += (mj - mbar) * (mj - mbar)
            W /= Mc
            B *= N / (Mc - 1.0)
            if ncold > 1 and nrec > 1 and W > 0.0:
                out["rhat"][k, cell] = np.float32(np.sqrt(((N - 1.0) / N * W + B / N) / W))
            h = (st["hist"][cs, k] * rep).astype(np.float64)
            lo, hi, tot = float(vmin[k, cell]), float(vmax[k, cell]), N * Mc
            for e, qv in enumerate((0.025, 0.5, 0.975)):
                target, cum, pos = qv * tot, 0.0, float(nbin)
                for b in range(nbin):
                    if h[b] > 0.0 and cum + h[b] >= target:
                        pos = b + (target - cum) / h[b]
                        break
                    cum += h[b]
                out["q"][e, k, cell] = np.float32(lo + pos * (hi - lo) / nbin)
            out["best"][k, cell] = st["best"][k, cs]
        a = int(st["accepted"][cols].sum())
        out["accept"][cell] = np.float32(a / (float(ndec) * Mc)) if ndec > 0 else np.float32(0)
        out["chi2_best"][cell] = np.float32(st["best_chi2"][cs])
    return out


def result(ns, wdat_cells, cells, ncell, nchain, ntemp):
    """dazim_mc_noise_result from a single-scale noise record: the one-group row of mc_groups_ref.result.  Returns dict lam_mean,
    lam_std [ncell] fp32 and ndata [ncell] int32."""
    r = mc_groups_ref.result(as_groups(ns, None, wdat_cells.shape[0]), wdat_cells, cells, ncell, nchain, ntemp)
    return {k: v[0] for k, v in r.items()}


def sample(forward, nburn, nsample, nadapt, gcell, nchain, vmin, vmax, vlast, cobs, wdat, nbin, seed, noise=None, prior=None, step0=0.05,
           ntemp=1, tmax=1.0, nswap=1, kind=0, each=None):
    """the whole sampler from the restatement alone, no library: vmin, vmax [nlay][ncs], vlast [ncs], cobs, wdat [kmax][ncs] fp32 of
    the sampled cells gcell; forward(prop [nz][ncol] fp32) -> curves [kmax][ncol] fp64.  noise: None (the fixed level), (a0, b0) (the
    single-scale record) or (grp, a0, b0) (the groups' record); prior: None or (smooth, damp, vref [nlay][ncs]); each(t, r) sees every
    step's returned dict.  Returns (state, ladder, noise record or None)."""
    nlay, ncs = vmin.shape
    ncol = ncs * nchain
    rep = lambda x: np.repeat(x, nchain, axis=-1)
    lo, hi = rep(vmin.astype(np.float64)), rep(vmax.astype(np.float64))
    cb, wd = rep(cobs), rep(wdat)
    _, _, _, gid = layout(ncol, nchain, ntemp, gcell)
    prop = np.concatenate([start_models(gid, lo, hi, seed), rep(vlast.astype(np.float32))[None]])
    st = dict(cur=prop.copy(), chi2=np.full(ncol, np.inf), scale=np.full(ncs, step0, np.float32), step=0,
              sums=np.zeros((2, nlay, ncol)), hist=np.zeros((ncs, nlay, nbin), np.uint32), accepted=np.zeros(ncol, np.int64),
              best=np.zeros((nlay, ncs), np.float32), best_chi2=np.full(ncs, np.inf))
    tp = dict(ntemp=ntemp, tmax=tmax, nswap=nswap)
    if ntemp > 1:
        tp.update(beta=ladder(ntemp, tmax), scale=np.full((ncs, ntemp), step0, np.float32),
                  swap_try=np.zeros((ncs, ntemp - 1), np.int64), swap_acc=np.zeros((ncs, ntemp - 1), np.int64))
    tp = ladder_state(st, tp)
    cov = empty_cov(ncs, nlay) if kind == 1 else None
    ns = None if noise is None else (empty_noise if len(noise) == 2 else empty_groups)(*noise, ncol)
    pr = None if prior is None else empty_prior(prior[0], prior[1], rep(prior[2]), prop)
    acc_win = np.zeros((ncs, ntemp), np.int64)
    nbd = 0
    for t in range(1, nburn + nsample + 1):
        record = t > nburn
        adapt = False
        if not record and t > 1:
            nbd += 1
            adapt = nbd % nadapt == 0
        r = step(st, tp, cov, ns, pr, prop, forward(prop), t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cb, wd, nbin, seed)
        st, tp, cov, ns, pr, acc_win = (r[k] for k in ("st", "tp", "cov", "ns", "pr", "acc_win"))
        if each:
            each(t, r)
        prop = proposals(st["cur"], tp["scale"], cov, prop, t, gcell, nchain, lo, hi, seed)
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
