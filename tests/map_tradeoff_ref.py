"""NumPy fp64 statements of dazim_map_tradeoff and dazim_map_tradeoff_total (include/dazim.h), the sweeps their
tests run and their problems: map_posterior_ref's shapes and regularisers with a right-hand side b = G x_true + unit noise.  `linalg` is
the independent reference (numpy.linalg.solve, slogdet and inv per point and period), `brute_evidence` the log marginal likelihood
log N(b_p; 0, I + G_p P^-1 G_p^T) without the closed form, `totals` the sums over the periods."""
import numpy as np

from tests import map_posterior_ref as mref
from tests import model_tradeoff_ref as tref

SCALES = tref.SCALES
DAMP_FACTORS = tref.DAMP_FACTORS
COND_MAX = tref.COND_MAX
PER_PERIOD = ("chi2", "reg2", "xnorm2", "logdet_a", "logdet_p", "dof", "gcv", "logev")
OUTPUTS = PER_PERIOD + ("x",)
TOTALS = ("chi2", "reg2sum", "dof", "gcv", "logev")


def seed_of(nx, ny, azim, kmax):
    return nx * 100 + ny + 7 * azim + kmax


def problem(nx, ny, kmax, azim, reg, **kw):
    """map_posterior_ref's problem of this shape and regulariser (the generator and seed of its tests) and b [m_data] fp32"""
    prob = mref.problem(nx, ny, kmax, azim, reg[0], reg[1], seed=seed_of(nx, ny, azim, kmax), **kw)
    return with_rhs(prob, seed_of(nx, ny, azim, kmax) + 12345)


def with_rhs(prob, seed):
    G = tref.dense(prob)[:prob["m_data"]]
    rng = np.random.default_rng(seed)
    x_true = rng.standard_normal(prob["n"])
    prob["b"] = (G @ x_true + rng.standard_normal(prob["m_data"])).astype(np.float32)
    return prob


def long_case(azim, reg, **kw):
    """mref.long_case with a right-hand side"""
    nx, ny = mref.LONG_SHAPES[azim]
    return with_rhs(mref.long_case(azim, reg, **kw), seed_of(nx, ny, azim, mref.LONG_KMAX) + 12345)


def without_data(prob, period):
    """the problem without the data rows of one period: their triplets are removed, the rows stay (empty) and keep their b"""
    ncell = (prob["nx"] - 2) * (prob["ny"] - 2)
    col, row = prob["icol"].astype(np.int64) - 1, prob["irow"].astype(np.int64) - 1
    keep = ~(((col % (prob["kmax"] * ncell)) // ncell == period) & (row < prob["m_data"]))
    return dict(prob, irow=prob["irow"][keep], icol=prob["icol"][keep], rw=prob["rw"][keep])


def sweep(prob, damp_factors=DAMP_FACTORS):
    """(scale [K][nblk], damp [K]) fp32: every scale on all blocks, with azim also on the a1/a2 blocks alone, crossed with the
    damping factors; the common-factor points of one damping factor are consecutive and ascend"""
    nblk = 3 if prob["azim"] else 1
    sc, dm = [], []
    for f in damp_factors:
        for s in SCALES:
            sc.append([s] * nblk)
            dm.append(f * prob["damp"])
        if prob["azim"]:
            for s in SCALES:
                sc.append([1.0, s, s])
                dm.append(f * prob["damp"])
    return np.array(sc, np.float32), np.array(dm, np.float32)


def periods(prob):
    """per period: G_p [m_p][n_g] and L_p (dense, ascending row order) in the local index blk*ncell + cell, b_p, and the block of
    every regularisation row (a row in two blocks is an error)"""
    kmax = prob["kmax"]
    ncell = (prob["nx"] - 2) * (prob["ny"] - 2)
    nblk = 3 if prob["azim"] else 1
    ng = nblk * ncell
    row, col, val = prob["irow"].astype(np.int64) - 1, prob["icol"].astype(np.int64) - 1, prob["rw"].astype(np.float64)
    per = (col % (kmax * ncell)) // ncell
    loc = (col // (kmax * ncell)) * ncell + col % ncell
    out = []
    for p in range(kmax):
        on = per == p
        rows = np.unique(row[on])
        assert not np.isin(row[~on], rows).any(), "a row in two periods"
        dense = np.zeros((len(rows), ng))
        np.add.at(dense, (np.searchsorted(rows, row[on]), loc[on]), val[on])
        nd = int((rows < prob["m_data"]).sum())
        L = dense[nd:]
        blk = np.zeros(len(L), np.int64)
        for l, r in enumerate(L):
            nz = np.flatnonzero(r)
            assert len(nz) and nz[0] // ncell == nz[-1] // ncell, "a regularisation row in two blocks"
            blk[l] = nz[0] // ncell
        out.append(dict(G=dense[:nd], L=L, blk=blk, b=prob["b"].astype(np.float64)[rows[:nd]]))
    return out


def prior(part, nblk, scale, damp):
    P = float(damp) ** 2 * np.eye(part["G"].shape[1])
    for b in range(nblk):
        Lb = part["L"][part["blk"] == b]
        P += float(scale[b]) ** 2 * (Lb.T @ Lb)
    return P


is_pd = tref.is_pd


def linalg(prob, scale, damp):
    """every output of Context.map_tradeoff in fp64 (x [K][n]); NaN at a (point, period) whose A is not positive definite"""
    kmax = prob["kmax"]
    ncell = (prob["nx"] - 2) * (prob["ny"] - 2)
    nblk = 3 if prob["azim"] else 1
    K = len(damp)
    nan = lambda *shape: np.full(shape, np.nan)
    out = dict(chi2=nan(K, kmax), reg2=nan(K, kmax, nblk), xnorm2=nan(K, kmax), logdet_a=nan(K, kmax), logdet_p=nan(K, kmax),
               dof=nan(K, kmax, nblk), gcv=nan(K, kmax), logev=nan(K, kmax), x=nan(K, nblk, kmax, ncell),
               n_failed=np.zeros((K, kmax), np.int32), mdata_p=np.zeros(kmax, np.int64))
    for p, part in enumerate(periods(prob)):
        G, L, blk, b = part["G"], part["L"], part["blk"], part["b"]
        mp = len(b)
        out["mdata_p"][p] = mp
        D, g = G.T @ G, G.T @ b
        for k in range(K):
            P = prior(part, nblk, scale[k], damp[k])
            A = D + P
            if not is_pd(A):
                out["n_failed"][k, p] = 1
                continue
            x = np.linalg.solve(A, g)
            C = np.linalg.inv(A)
            out["x"][k, :, p] = x.reshape(nblk, ncell)
            chi2 = out["chi2"][k, p] = np.sum((G @ x - b) ** 2)
            reg2 = out["reg2"][k, p] = [np.sum((L[blk == bb] @ x) ** 2) for bb in range(nblk)]
            out["xnorm2"][k, p] = x @ x
            out["logdet_a"][k, p] = np.linalg.slogdet(A)[1]
            if is_pd(P):
                out["logdet_p"][k, p] = np.linalg.slogdet(P)[1]
            dof = out["dof"][k, p] = (C * D).sum(axis=1).reshape(nblk, ncell).sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                out["gcv"][k, p] = np.float64(mp * chi2) / np.float64(mp - dof.sum()) ** 2
            J = float(np.sum(scale[k].astype(np.float64) ** 2 * reg2) + float(damp[k]) ** 2 * out["xnorm2"][k, p])
            out["logev"][k, p] = -0.5 * (chi2 + J) + 0.5 * out["logdet_p"][k, p] - 0.5 * out["logdet_a"][k, p] - 0.5 * mp * np.log(2 * np.pi)
    out["x"] = out["x"].reshape(K, -1)
    return out


def totals(out):
    """dazim_map_tradeoff_total: the sums over the periods, and the GCV of the whole system"""
    M = float(out["mdata_p"].sum())
    chi2, dof = out["chi2"].sum(axis=1), out["dof"].sum(axis=(1, 2))
    return dict(chi2=chi2, reg2sum=out["reg2"].sum(axis=(1, 2)), dof=dof, gcv=M * chi2 / (M - dof) ** 2, logev=out["logev"].sum(axis=1))


def brute_evidence(G, b, P):
    """log N(b; 0, I + G P^-1 G^T): b = G x + e with x ~ N(0, P^-1), e ~ N(0, I)"""
    S = np.eye(len(b)) + G @ np.linalg.solve(P, G.T)
    return -0.5 * b @ np.linalg.solve(S, b) - 0.5 * np.linalg.slogdet(S)[1] - 0.5 * len(b) * np.log(2 * np.pi)


def worst(got, ref, keys=OUTPUTS):
    return tref.worst(got, ref, keys)
