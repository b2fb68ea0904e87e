"""NumPy fp64 statements of dazim_column_lsq_radial and dazim_column_resolution_radial: per cell the Vsv and
Vsh updates x = [xv; xh] of

    ||Wv (Kv xv - rv)||^2 + ||Wh (Kh xh - rh)||^2 + s^2 (||L xv||^2 + ||L xh||^2) + d^2 ||x||^2 + mu^2 ||xh - xv + d0||^2

`solve` is the stacked system [Wv Kv, 0; 0, Wh Kh; sL, 0; 0, sL; dI, 0; 0, dI; -mu I, mu I] x = [Wv rv; Wh rh; 0; 0; 0; 0; -mu d0]
through numpy.linalg.lstsq, `linalg` the posterior through numpy.linalg.inv, and `route` the kernel's own way (packed lower triangle,
Cholesky, inverse factor and C = M^T M in place, lane by lane and barrier by barrier) for the CPU test of that plan.  Each takes
one cell; `per_cell_solve` and `per_cell_res` run them over the inner cells of kernel tables laid out as the entries read them."""
import numpy as np

from tests.test_column_lsq_gpu import depth_rule, random_problem

PER_KNOT = ("std", "rdiag", "rsum", "cross")
OUTPUTS = PER_KNOT + ("cov_vh", "trace", "rows")


def f32(v):
    """a regulariser as the C entry receives it"""
    return float(np.float32(v))


def penalty2(n, smooth, damp, couple):
    """P2 = [[P + mu^2 I, -mu^2 I], [-mu^2 I, P + mu^2 I]], P = smooth^2 L^T L + damp^2 I"""
    s, d, m = f32(smooth), f32(damp), f32(couple)
    L = depth_rule(n)
    P = s * s * (L.T @ L) + d * d * np.eye(n)
    I = np.eye(n)
    return np.block([[P + m * m * I, -m * m * I], [-m * m * I, P + m * m * I]])


def data_matrix(Kv, wv, Kh, wh):
    """blockdiag(Kv^T Wv^2 Kv, Kh^T Wh^2 Kh)"""
    n = Kv.shape[1]
    N = np.zeros((2 * n, 2 * n))
    N[:n, :n] = (Kv * (wv * wv)[:, None]).T @ Kv
    N[n:, n:] = (Kh * (wh * wh)[:, None]).T @ Kh
    return N


def solve(Kv, wv, rv, Kh, wh, rh, d0, smooth, damp, couple):
    """x [2n] of one cell from the stacked system: Kv [kv][n], Kh [kh][n] (kv or kh may be 0), d0 [n]"""
    n = Kv.shape[1]
    s, d, m = f32(smooth), f32(damp), f32(couple)
    L, I, Z = depth_rule(n), np.eye(n), np.zeros((n, n))
    A = np.vstack([np.hstack([wv[:, None] * Kv, np.zeros((len(wv), n))]), np.hstack([np.zeros((len(wh), n)), wh[:, None] * Kh]),
                   np.hstack([s * L, Z]), np.hstack([Z, s * L]), np.hstack([d * I, Z]), np.hstack([Z, d * I]), np.hstack([-m * I, m * I])])
    b = np.concatenate([wv * rv, wh * rh, np.zeros(4 * n), -m * d0])
    return np.linalg.lstsq(A, b, rcond=None)[0]


def derived(C, Rm):
    n = len(C) // 2
    a = np.abs(Rm)
    other = np.concatenate([a[:n, n:].sum(axis=1), a[n:, :n].sum(axis=1)])
    den = a.sum(axis=1)
    return dict(std=np.sqrt(np.diag(C)), cov_vh=np.diag(C[:n, n:]).copy(), rdiag=np.diag(Rm).copy(), rsum=Rm.sum(axis=1),
                cross=np.where(den > 0, other / np.where(den > 0, den, 1.0), 0.0), trace=np.array([np.trace(Rm[:n, :n]), np.trace(Rm[n:, n:])]),
                rows=Rm)


def linalg(Kv, wv, Kh, wh, smooth, damp, couple):
    """the independent reference: C = numpy.linalg.inv(A) and Rm = I - C P2 in the form C blockdiag(Kv^T Wv^2 Kv, Kh^T Wh^2 Kh), as
    column_res_ref.linalg forms it: the difference loses what is small against |C| |P2| (nlay 32, one Rayleigh period, no Love data,
    smoothing alone, couple 50: the Love columns of Rm are exactly 0 in the product and 4e-8 in the difference, which `cross` then
    divides by a row sum of 0.026)"""
    n = Kv.shape[1]
    N = data_matrix(Kv, wv, Kh, wh)
    C = np.linalg.inv(N + penalty2(n, smooth, damp, couple))
    return derived(C, C @ N)


def tri(a, c):
    return a * (a + 1) // 2 + c


def route(Kv, wv, Kh, wh, smooth, damp, couple, rhs=None):
    """the kernel's plan on one cell: A as a packed lower triangle, every step in place, a lane's reads of a step all before the
    step's writes (the barriers).  Returns the outputs of `linalg`, or None at a pivot that is not finite and > 0; with rhs = b [2n]
    the solution of A x = b instead."""
    n = Kv.shape[1]
    N = 2 * n
    full = data_matrix(Kv, wv, Kh, wh) + penalty2(n, smooth, damp, couple)
    A = np.zeros(N * (N + 1) // 2)
    for a in range(N):
        for c in range(a + 1):
            A[tri(a, c)] = full[a, c]
    for c in range(N):                                   # potrf
        p = A[tri(c, c)]
        if not (np.isfinite(p) and p > 0):
            return None
        d = np.sqrt(p)
        for t in range(c + 1, N):
            A[tri(t, c)] /= d
        A[tri(c, c)] = d
        for t in range(c + 1, N):
            for e in range(c + 1, t + 1):
                A[tri(t, e)] -= A[tri(t, c)] * A[tri(e, c)]
    if rhs is not None:
        b = np.array(rhs, np.float64)
        for c in range(N):
            b[c] /= A[tri(c, c)]
            for t in range(c + 1, N):
                b[t] -= A[tri(t, c)] * b[c]
        for c in range(N - 1, -1, -1):
            b[c] /= A[tri(c, c)]
            for t in range(c):
                b[t] -= A[tri(c, t)] * b[c]
        return b
    for c in range(N - 1, -1, -1):                       # trtri
        inv = 1.0 / A[tri(c, c)]
        v = [-sum(A[tri(t, l)] * A[tri(l, c)] for l in range(c + 1, t + 1)) * inv for t in range(c + 1, N)]
        for t in range(c + 1, N):
            A[tri(t, c)] = v[t - c - 1]
        A[tri(c, c)] = inv
    for a in range(N):                                   # lauum
        s = [sum(A[tri(q, a)] * A[tri(q, t)] for q in range(a, N)) for t in range(a + 1)]
        for t in range(a + 1):
            A[tri(a, t)] = s[t]
    C = np.zeros((N, N))
    for a in range(N):
        for c in range(a + 1):
            C[a, c] = C[c, a] = A[tri(a, c)]
    return derived(C, np.eye(N) - C @ penalty2(n, smooth, damp, couple))


def cell_slices(nx, ny, nlay, kern, wdat, c):
    """(K [k][nlay] with the rows without data zeroed, w [k]) of inner cell c; a table that is None has no periods"""
    if kern is None:
        return np.zeros((0, nlay)), np.zeros(0)
    k = kern.shape[1]
    ncell = (nx - 2) * (ny - 2)
    w = np.ones(k) if wdat is None else np.asarray(wdat).reshape(k, ncell)[:, c].astype(np.float64)
    col = (c // (nx - 2) + 1) * nx + c % (nx - 2) + 1
    K = kern[:nlay, :, col].T.astype(np.float64)
    K[w == 0] = 0.0                                      # (a period without data is not read)
    return K, w


def per_cell_solve(nx, ny, nlay, kern_v, kern_h, rhs_v, rhs_h, w_v, w_h, d0, smooth, damp, couple):
    """`solve` over the inner cells: x [2][nlay][ncell], the cells without data left at 0; their number; and the RMS over the cells
    with w != 0 of r and of r - K x per period, [kv + kh][2], the Rayleigh periods first"""
    ncell = (nx - 2) * (ny - 2)
    kv, kh = (0 if k is None else k.shape[1] for k in (kern_v, kern_h))
    x = np.zeros((2, nlay, ncell))
    ss, cnt, n_empty = np.zeros((kv + kh, 2)), np.zeros(kv + kh), 0
    rv = np.zeros((0, ncell)) if kv == 0 else np.asarray(rhs_v).reshape(kv, ncell).astype(np.float64)
    rh = np.zeros((0, ncell)) if kh == 0 else np.asarray(rhs_h).reshape(kh, ncell).astype(np.float64)
    d = np.zeros((nlay, ncell)) if d0 is None else np.asarray(d0).reshape(nlay, ncell).astype(np.float64)
    for c in range(ncell):
        Kv, wv = cell_slices(nx, ny, nlay, kern_v, w_v, c)
        Kh, wh = cell_slices(nx, ny, nlay, kern_h, w_h, c)
        on = np.concatenate([wv, wh]) != 0
        if not on.any():
            n_empty += 1
            continue
        xc = solve(Kv, wv, rv[:, c], Kh, wh, rh[:, c], d[:, c], smooth, damp, couple)
        x[:, :, c] = xc.reshape(2, nlay)
        r = np.concatenate([rv[:, c], rh[:, c]])
        res = r - np.concatenate([Kv @ xc[:nlay], Kh @ xc[nlay:]])
        cnt += on
        ss[on, 0] += r[on] ** 2
        ss[on, 1] += res[on] ** 2
    return x, n_empty, np.sqrt(ss / np.maximum(cnt, 1)[:, None])


def per_cell_res(fn, nx, ny, nlay, kern_v, kern_h, w_v, w_h, smooth, damp, couple):
    """fn (`linalg` or `route`) over the inner cells: std, rdiag, rsum, cross [2 nlay][ncell], cov_vh [nlay][ncell], trace [2][ncell],
    rows [2 nlay][2 nlay][ncell], all 0 in a cell without data and NaN where fn gives up; n_empty and n_failed"""
    ncell, N = (nx - 2) * (ny - 2), 2 * nlay
    out = {k: np.zeros((N, ncell)) for k in PER_KNOT}
    out.update(cov_vh=np.zeros((nlay, ncell)), trace=np.zeros((2, ncell)), rows=np.zeros((N, N, ncell)), n_empty=0, n_failed=0)
    for c in range(ncell):
        Kv, wv = cell_slices(nx, ny, nlay, kern_v, w_v, c)
        Kh, wh = cell_slices(nx, ny, nlay, kern_h, w_h, c)
        if not (np.concatenate([wv, wh]) != 0).any():
            out["n_empty"] += 1
            continue
        one = fn(Kv, wv, Kh, wh, smooth, damp, couple)
        if one is None:
            out["n_failed"] += 1
        for k in OUTPUTS:
            out[k][..., c] = np.nan if one is None else one[k]
    return out


def radial_problem(nx, ny, nlay, kv, kh, seed):
    """kernels, right-hand sides and weights of both blocks drawn as random_problem draws them (None for a block without periods), and
    a random d0.  Cell 3 has no data in either block; cell 5 a single period in all (the last Rayleigh one, or the last Love one
    when kv = 0); cell 7 Love data only (when there are Love periods)."""
    rng = np.random.default_rng(seed + 5)
    blocks = []
    for q, k in enumerate((kv, kh)):
        blocks.append(random_problem(nx, ny, nlay, k, 1, 0, seed=seed * 2 + q) if k else (None, None, None))
    (kern_v, rhs_v, w_v), (kern_h, rhs_h, w_h) = blocks
    if kv and kh:
        w_h.reshape(kh, -1)[:, 5] = 0.0
        w_v.reshape(kv, -1)[:, 7] = 0.0
        w_h.reshape(kh, -1)[0, 7] = 1.5
    d0 = (0.2 * rng.standard_normal((nlay, ny - 2, nx - 2))).astype(np.float32)
    return kern_v, kern_h, None if rhs_v is None else rhs_v[0], None if rhs_h is None else rhs_h[0], w_v, w_h, d0


def worst(got, ref, keys=OUTPUTS):
    """per output the largest over the cells of max |got - ref| / max(1, max |ref|), each maximum taken within the cell"""
    res = {}
    for k in keys:
        g = np.asarray(got[k], np.float64).reshape(-1, ref[k].shape[-1])
        r = ref[k].reshape(-1, ref[k].shape[-1])
        res[k] = float((np.abs(g - r).max(axis=0) / np.maximum(1.0, np.abs(r).max(axis=0))).max())
    return res
