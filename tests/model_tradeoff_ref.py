"""NumPy fp64 statements of dazim_model_tradeoff (include/dazim.h), the sweeps its tests run and their problems:
model_posterior_ref's shapes and regularisers with a right-hand side b = G x_true + unit noise.  `linalg` is the independent reference
(numpy.linalg.solve, slogdet and inv per point on the D, L of model_posterior_ref.parts), `brute_evidence` the log marginal likelihood
log N(b; 0, I + G P^-1 G^T) without the closed form, `pick` the three rules of dazim_tradeoff_pick."""
import numpy as np

from tests import dense_ref
from tests import model_posterior_ref as mref

SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
DAMP_FACTORS = (0.5, 1.0, 2.0)
OUTPUTS = ("chi2", "reg2", "xnorm2", "logdet_a", "logdet_p", "dof", "gcv", "logev", "x")
COND_MAX = 1e4    # cond(A_k), and cond(P_k) where P_k is positive definite, of every point (tests/test_model_tradeoff_ref_cpu.py)


def seed_of(shape, joint):
    return shape[0] * 10000 + shape[1] * 100 + shape[2] + 7 * joint


def problem(shape, joint, reg):
    """model_posterior_ref's problem of this shape and regulariser (the generator and seed of its tests) and b [m_data] fp32"""
    prob = mref.problem(shape[0], shape[1], shape[2], joint, reg[0], reg[1], seed=seed_of(shape, joint))
    return with_rhs(prob, seed_of(shape, joint) + 12345)


def with_rhs(prob, seed):
    """b [m_data] fp32 = G x_true + unit noise on a ready problem (of `problem`'s or of mref.long_rows')"""
    G = dense(prob)[:prob["m_data"]]
    rng = np.random.default_rng(seed)
    x_true = rng.standard_normal(prob["n"])
    prob["b"] = (G @ x_true + rng.standard_normal(prob["m_data"])).astype(np.float32)
    return prob


def long_case(joint, reg):
    """mref.long_case with a right-hand side"""
    return with_rhs(mref.long_case(joint, reg), seed_of(mref.LONG_SHAPES[joint], joint) + 12345)


def sweep(prob, damp_factors=DAMP_FACTORS):
    """(scale [K][nblk], damp [K]) fp32: every scale on all blocks, in joint mode also on the Gc/Gs blocks alone, crossed with the
    damping factors; the common-factor points of one damping factor are consecutive and ascend"""
    nblk = 3 if prob["joint"] else 1
    sc, dm = [], []
    for f in damp_factors:
        for s in SCALES:
            sc.append([s] * nblk)
            dm.append(f * prob["damp"])
        if prob["joint"]:
            for s in SCALES:
                sc.append([1.0, s, s])
                dm.append(f * prob["damp"])
    return np.array(sc, np.float32), np.array(dm, np.float32)


def dense(prob):
    row, col, val = prob["irow"].astype(np.int64) - 1, prob["icol"].astype(np.int64) - 1, prob["rw"].astype(np.float64)
    out = np.zeros((prob["m"], prob["n"]))
    np.add.at(out, (row, col), val)
    return out


def blocks(prob, L):
    """the block of every regularisation row (that of its first entry; -1 for an empty row); a row in two blocks is an error"""
    nblk = 3 if prob["joint"] else 1
    maxvp = prob["n"] // nblk
    blk = np.full(len(L), -1)
    for l, r in enumerate(L):
        nz = np.flatnonzero(r)
        if len(nz):
            assert nz[0] // maxvp == nz[-1] // maxvp
            blk[l] = nz[0] // maxvp
    return blk


def prior(prob, L, blk, scale, damp):
    nblk = 3 if prob["joint"] else 1
    P = float(damp) ** 2 * np.eye(prob["n"])
    for b in range(nblk):
        Lb = L[blk == b]
        P += float(scale[b]) ** 2 * (Lb.T @ Lb)
    return P


def is_pd(A):
    try:
        np.linalg.cholesky(A)
        return True
    except np.linalg.LinAlgError:
        return False


def linalg(prob, scale, damp):
    """every output of Context.model_tradeoff in fp64 (x [K][n]); NaN at a point whose A_k is not positive definite"""
    nblk = 3 if prob["joint"] else 1
    n, md = prob["n"], prob["m_data"]
    maxvp = n // nblk
    D, L = mref.parts(prob)
    G = dense(prob)[:md]
    b = prob["b"].astype(np.float64)
    g = G.T @ b
    blk = blocks(prob, L)
    K = len(damp)
    out = dict(chi2=np.full(K, np.nan), reg2=np.full((K, nblk), np.nan), xnorm2=np.full(K, np.nan), logdet_a=np.full(K, np.nan),
               logdet_p=np.full(K, np.nan), dof=np.full((K, nblk), np.nan), gcv=np.full(K, np.nan), logev=np.full(K, np.nan),
               x=np.full((K, n), np.nan), n_failed=np.zeros(K, np.int32))
    for k in range(K):
        P = prior(prob, L, blk, scale[k], damp[k])
        A = D + P
        if not is_pd(A):
            out["n_failed"][k] = 1
            continue
        x = np.linalg.solve(A, g)
        C = np.linalg.inv(A)
        out["x"][k] = x
        out["chi2"][k] = np.sum((G @ x - b) ** 2)
        out["reg2"][k] = [np.sum((L[blk == bb] @ x) ** 2) for bb in range(nblk)]
        out["xnorm2"][k] = x @ x
        out["logdet_a"][k] = np.linalg.slogdet(A)[1]
        if is_pd(P):
            out["logdet_p"][k] = np.linalg.slogdet(P)[1]
        out["dof"][k] = (C * D).sum(axis=1).reshape(nblk, maxvp).sum(axis=1)
        out["gcv"][k] = md * out["chi2"][k] / (md - out["dof"][k].sum()) ** 2
        J = float(np.sum(scale[k].astype(np.float64) ** 2 * out["reg2"][k]) + float(damp[k]) ** 2 * out["xnorm2"][k])
        out["logev"][k] = -0.5 * (out["chi2"][k] + J) + 0.5 * out["logdet_p"][k] - 0.5 * out["logdet_a"][k] - 0.5 * md * np.log(2 * np.pi)
    return out


def brute_evidence(prob, scale, damp):
    """log N(b; 0, I + G P^-1 G^T): b = G x + e with x ~ N(0, P^-1), e ~ N(0, I)"""
    D, L = mref.parts(prob)
    G = dense(prob)[:prob["m_data"]]
    b = prob["b"].astype(np.float64)
    P = prior(prob, L, blocks(prob, L), scale, damp)
    S = np.eye(len(b)) + G @ np.linalg.solve(P, G.T)
    return -0.5 * b @ np.linalg.solve(S, b) - 0.5 * np.linalg.slogdet(S)[1] - 0.5 * len(b) * np.log(2 * np.pi)


def pick(chi2, reg2sum, gcv, logev):
    """dazim_tradeoff_pick's three rules: the first index of the smallest finite gcv, of the largest finite logev, and of the largest
    Menger curvature over the interior points of the polyline (log chi2, log reg2sum) through the finite points"""
    def first_best(a, sign):
        if a is None:
            return -1
        a = np.asarray(a, np.float64)
        ok = np.flatnonzero(np.isfinite(a))
        return int(ok[np.argmax(sign * a[ok])]) if len(ok) else -1
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = np.log(np.asarray(chi2, np.float64)), np.log(np.asarray(reg2sum, np.float64))
    ok = np.flatnonzero(np.isfinite(u) & np.isfinite(v))
    corner = -1
    if len(ok) >= 3:
        p = np.stack([u[ok], v[ok]], axis=1)
        a, b, c = p[1:-1] - p[:-2], p[2:] - p[1:-1], p[2:] - p[:-2]
        den = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) * np.linalg.norm(c, axis=1)
        curv = np.where(den > 0, 2 * np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]) / np.where(den > 0, den, 1.0), 0.0)
        corner = int(ok[1 + np.argmax(curv)])
    return dict(corner=corner, gcv=first_best(gcv, -1.0), evidence=first_best(logev, 1.0))


def check_pick(fn):
    """fn(chi2, reg2sum, gcv, logev) against `pick` on sweeps with NaN, infinite and zero entries, ties, fewer than three finite
    points and none"""
    rng = np.random.default_rng(3)
    for trial in range(200):
        K = int(rng.integers(1, 12))
        chi2, reg = np.exp(rng.normal(size=K)), np.exp(rng.normal(size=K))
        gcv, logev = rng.normal(size=K).round(1), rng.normal(size=K).round(1)     # (rounded: ties happen)
        for a in (chi2, reg, gcv, logev):
            a[rng.random(K) < 0.2] = rng.choice([np.nan, np.inf, -np.inf, 0.0])
        assert fn(chi2, reg, gcv, logev) == pick(chi2, reg, gcv, logev), (chi2, reg, gcv, logev)
    assert fn(np.ones(4), np.ones(4), None, None) == dict(corner=1, gcv=-1, evidence=-1)
    assert fn(np.ones(2), np.ones(2), np.ones(2), np.ones(2)) == dict(corner=-1, gcv=0, evidence=0)


def worst(got, ref, keys=OUTPUTS):
    """dense_ref.worst with every output taken in the reference's layout (x [K][n], and the maps' arrays against the model's)"""
    return dense_ref.worst(got, ref, keys, reshaped=keys)
