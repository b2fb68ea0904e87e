"""NumPy restatement of the Monte-Carlo step of dazim_mc (include/dazim.h): Philox4x32-10, the draws, and one
step from a copy of the chain state.  Every operation is the library's in the same order and precision (the library is compiled
without FMA contraction); only log, sqrt, cos and sin may differ in the last bit."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
TWO_PI = 6.283185307179586
MAXFOLD = 8     # reflections of a proposal into its box (4 always suffice for a step scale <= 0.5)


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


def step(st, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cobs, wdat, nbin, seed):
    """one step from the state `st` (dict of MonteCarlo.state()) and the proposals prop [nz][ncol]; gcell [ncs] the inner-cell index
    of each sampled cell; lo, hi [nlay][ncol] fp64 and cobs, wdat [kmax][ncol] per column; acc_win [ncs] the burn-in window counts.
    Returns (new state dict, accept decisions [ncol], next proposals [nz][ncol], acc_win)."""
    nz, ncol = prop.shape
    nlay = nz - 1
    ncs = ncol // nchain
    cs = np.repeat(np.arange(ncs), nchain)
    gid = (gcell[cs] * nchain + np.tile(np.arange(nchain), ncs)).astype(np.uint32)
    chi2p = chi2(pv, cobs, wdat)
    first = t == 1
    if first:
        acc = np.ones(ncol, bool)
    else:
        c = st["chi2"]
        u = uniform(block(t, gid, 0, seed)[..., 0])
        with np.errstate(invalid="ignore"):
            acc = np.where(np.isinf(c), ~np.isinf(chi2p), np.log(u) < -0.5 * (chi2p - c))
    cur = st["cur"].copy()
    cur[:nlay, acc] = prop[:nlay, acc]
    ch2 = np.where(acc, chi2p, st["chi2"])
    nacc = np.zeros(ncs, np.int64) if first else np.bincount(cs, weights=acc, minlength=ncs).astype(np.int64)
    scale = st["scale"].copy()
    sums, hist, accepted = st["sums"].copy(), st["hist"].copy(), st["accepted"].copy()
    best, best_chi2 = st["best"].copy(), st["best_chi2"].copy()
    acc_win = acc_win.copy()
    if not record:
        acc_win += nacc
        if adapt:
            rate = acc_win.astype(np.float64) / (float(nadapt) * float(nchain))
            up, down = rate > 0.40, rate < 0.20
            s = np.where(up, scale * np.float32(1.25), np.where(down, scale / np.float32(1.25), scale)).astype(np.float32)
            scale = np.minimum(np.maximum(s, np.float32(1e-3)), np.float32(0.5)).astype(np.float32)
            acc_win[:] = 0
    else:
        if not first:
            accepted += acc
        # the lowest chi2 of the step per cell, the first chain on ties; it replaces the best only when strictly lower
        c2 = ch2.reshape(ncs, nchain)
        win = np.argmin(c2, axis=1)
        m = c2[np.arange(ncs), win]
        upd = m < best_chi2
        wcol = np.arange(ncs) * nchain + win
        best[:, upd] = cur[:nlay, wcol[upd]]
        best_chi2 = np.where(upd, m, best_chi2)
        v = cur[:nlay].astype(np.float64)
        sums[0] += v
        sums[1] += v * v
        b = ((v - lo) / (hi - lo) * float(nbin)).astype(np.int64)
        b = np.clip(b, 0, nbin - 1)
        for k in range(nlay):
            np.add.at(hist, (cs, k, b[k]), 1)
    z = normals(t, gid, nlay, seed)
    d = scale[cs].astype(np.float64) * (hi - lo)
    v = cur[:nlay].astype(np.float64) + d * z
    for _ in range(MAXFOLD):
        below, above = v < lo, v > hi
        if not (below | above).any():
            break
        v = np.where(below, 2.0 * lo - v, np.where(above, 2.0 * hi - v, v))
    nxt = prop.copy()
    nxt[:nlay] = np.minimum(np.maximum(v, lo), hi).astype(np.float32)
    new = dict(cur=cur, chi2=ch2, scale=scale, step=t, sums=sums, hist=hist, accepted=accepted, best=best, best_chi2=best_chi2)
    return new, acc, nxt, acc_win


def final(st, vmin, vmax, vel0_knots, cells, ncell, nchain, nrec, ndec, nbin):
    """k_mc_final from a state: vmin, vmax, vel0_knots [nlay][ncell] fp32 (the inner cells), cells the sampled inner-cell indices.
    Returns dict mean, std, q [3][nlay][ncell], best, rhat, accept, chi2_best as the library forms them (fp32)."""
    nlay = vmin.shape[0]
    out = dict(mean=vel0_knots.copy(), std=np.zeros((nlay, ncell), np.float32), q=np.stack([vel0_knots] * 3), best=vel0_knots.copy(),
               rhat=np.full((nlay, ncell), np.nan, np.float32), accept=np.zeros(ncell, np.float32),
               chi2_best=np.zeros(ncell, np.float32))
    N, Mc = float(nrec), float(nchain)
    for cs, cell in enumerate(cells):
        cols = cs * nchain + np.arange(nchain)
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
            if nchain > 1 and nrec > 1 and W > 0.0:
                out["rhat"][k, cell] = np.float32(np.sqrt(((N - 1.0) / N * W + B / N) / W))
            h = st["hist"][cs, k].astype(np.float64)
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
