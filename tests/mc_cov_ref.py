"""NumPy restatement of the covariance-adapted proposal of dazim_mc (proposal kind 1 in include/dazim.h) as
additions to tests/mc_ref.py's step: the sums over the burn-in states, the factor at the adaptation points, the scale range and the
proposals y = L z.  Every operation is the library's in the same order and precision; only log, sqrt, cos and sin may differ in the
last bit."""
import numpy as np

from tests import mc_ref

COV_MIN = 8          # states per knot before a window factors
RIDGE = 1e-8


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


def step(st, cov, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cobs, wdat, nbin, seed):
    """one kind-1 step from the state `st` (MonteCarlo.state()) and `cov` (MonteCarlo.cov_state()); the other arguments are
    mc_ref.step's.  Returns (new state, new cov with the restated factor, accept decisions, acc_win, {cs: C} of the cells factored in
    this step).  The next proposals come from proposals(), so that a test can form them from the library's factor."""
    nz, ncol = prop.shape
    nlay = nz - 1
    ncs = ncol // nchain
    new, acc, _, acc_win2 = mc_ref.step(st, prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cobs, wdat, nbin, seed)
    cov = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cov.items()}
    set0 = cov["cov_set"].copy()
    first = t == 1
    factored = {}
    root = np.sqrt(np.float32(nlay))
    if not record and adapt:
        # the scale rule again, with the range of the cells that have a factor
        nacc = np.bincount(np.repeat(np.arange(ncs), nchain), weights=acc, minlength=ncs).astype(np.int64)
        rate = (acc_win + nacc).astype(np.float64) / (float(nadapt) * float(nchain))
        s0 = st["scale"]
        s = np.where(rate > 0.40, s0 * np.float32(1.25), np.where(rate < 0.20, s0 / np.float32(1.25), s0)).astype(np.float32)
        cap = np.where(set0 == 1, np.float32(2.0) / root, np.float32(0.5)).astype(np.float32)
        new["scale"] = np.minimum(np.maximum(s, np.float32(1e-3)), cap).astype(np.float32)
    if not record and not first:
        u = (new["cur"][:nlay].astype(np.float64) - lo) / (hi - lo)
        a, c = pairs(nlay)
        for cs in range(ncs):
            for ch in range(nchain):
                col = cs * nchain + ch
                cov["cov_s1"][cs] += u[:, col]
                cov["cov_s2"][cs] += u[a, col] * u[c, col]
            cov["cov_n"][cs] += nchain
        if adapt:
            for cs in range(ncs):
                if cov["cov_n"][cs] < COV_MIN * nlay:
                    continue
                C = covariance(cov["cov_n"][cs], cov["cov_s1"][cs], cov["cov_s2"][cs], nlay)
                ok, L = cholesky(C)
                factored[cs] = C
                if ok:
                    cov["chol"][cs] = L
                    if set0[cs] == 0:
                        cov["cov_set"][cs] = 1
                        new["scale"][cs] = np.float32(1.0) / root
                cov["cov_n"][cs] = 0
                cov["cov_s1"][cs] = 0.0
                cov["cov_s2"][cs] = 0.0
    return new, cov, acc, acc_win2, factored


def proposals(cur, scale, chol, cov_set, prop, t, gcell, nchain, lo, hi, seed):
    """the proposals after step t from the state cur [nz][ncol], the scales, the packed factors chol [ncs][npair] and cov_set"""
    nz, ncol = prop.shape
    nlay = nz - 1
    ncs = ncol // nchain
    cs = np.repeat(np.arange(ncs), nchain)
    gid = (gcell[cs] * nchain + np.tile(np.arange(nchain), ncs)).astype(np.uint32)
    z = mc_ref.normals(t, gid, nlay, seed)
    y = z.copy()
    on = cov_set[cs] == 1
    for k in range(nlay):
        yk = np.zeros(ncol)
        for j in range(k + 1):
            yk = yk + chol[cs, k * (k + 1) // 2 + j] * z[j]
        y[k] = np.where(on, yk, z[k])
    d = scale[cs].astype(np.float64) * (hi - lo)
    v = cur[:nlay].astype(np.float64) + d * y
    for _ in range(mc_ref.MAXFOLD):
        below, above = v < lo, v > hi
        if not (below | above).any():
            break
        v = np.where(below, 2.0 * lo - v, np.where(above, 2.0 * hi - v, v))
    nxt = prop.copy()
    nxt[:nlay] = np.minimum(np.maximum(v, lo), hi).astype(np.float32)
    return nxt
