"""NumPy fp64 statements of dazim_map_posterior (include/dazim.h) from COO triplets, and the problems its tests
run on.  `linalg` is the independent reference (numpy.linalg.inv of every period's normal matrix, Rm = C D), `route` follows the
kernels (right-looking Cholesky, M = R^-1 by forward substitution, C = M^T M, Rm = I - C P with the regularisation rows applied one
by one and the damping last).  Both return the arrays of Context.map_posterior in fp64."""
import numpy as np

from tests import dense_ref

PER_UNKNOWN = ("std_post", "std_noise", "rdiag", "rsum", "width", "leak")
OUTPUTS = PER_UNKNOWN + ("trace", "rows")

NB = 32   # the panel width of the factorisation (stat map_post.nb): the sizes below sit on both sides of one, two and four panels
# (nx, ny) with n_g = ncell = 1, NB-1, NB, NB+1, 2NB+1 and 135 (>= 4NB+3, no multiple of 16)
SHAPES_ISO = [(3, 3), (33, 3), (10, 6), (13, 5), (15, 7), (17, 11)]
# n_g = 3 ncell: NB-1, NB and 2NB+1 are no multiples of 3, so 30 and 33 (= NB+1), 63 and 66 stand on both sides of the panel edges;
# 3, and 135 = 3 * 45 (ncell no multiple of 4)
SHAPES_JOINT = [(3, 3), (12, 3), (13, 3), (9, 5), (13, 4), (11, 7)]
REGS = [(0.7, 0.3), (0.0, 0.5), (0.8, 0.0)]
REG_IDS = ["smooth+damp", "damp", "smooth"]


def laplacian2d(nx, ny, weights):
    """the rows of dazim_csr_append_laplacian2d as 0-based (row, col, value) triplets: map b on columns b*ncell .., weight weights[b];
    a cell on an edge of the map the single entry 2w, an inner cell 4w and -w on its four neighbours; rows in map, j, i order"""
    nvx, nvy = nx - 2, ny - 2
    ncell = nvx * nvy
    r, c, v = [], [], []
    for b, w in enumerate(np.asarray(weights, np.float32)):
        for cell in range(ncell):
            j, i = divmod(cell, nvx)
            row, col = b * ncell + cell, b * ncell + cell
            if i in (0, nvx - 1) or j in (0, nvy - 1):
                r.append(row); c.append(col); v.append(np.float32(2.0) * w)
            else:
                for d, f in ((-nvx, -1.0), (-1, -1.0), (0, 4.0), (1, -1.0), (nvx, -1.0)):
                    r.append(row); c.append(col + d); v.append(np.float32(f) * w)
    return np.array(r, np.int64), np.array(c, np.int64), np.array(v, np.float32)


def problem(nx, ny, kmax, azim, smooth, damp, seed=0, rays_per_period=None, no_reg_period=None):
    """random sparse data rows, each confined to one period (the periods interleaved row by row; with azim a row holds the c, a1
    and a2 columns of its cells, as a ray does), the regularisation rows of laplacian2d with weight `smooth` on every map (none for
    smooth = 0, none for period no_reg_period) and the damping.  The last cell of the map is crossed by no row (when there is more
    than one cell).  Triplets 1-based, as Context.csr_from_coo takes them; the values are fp32."""
    rng = np.random.default_rng(seed)
    nvx, nvy = nx - 2, ny - 2
    ncell, nblk = nvx * nvy, 3 if azim else 1
    live = max(ncell - 1, 1)
    nray = rays_per_period if rays_per_period is not None else 2 * ncell + 3
    m_data = nray * kmax
    period = rng.permutation(np.arange(m_data) % kmax)
    r, c, v = [], [], []
    for row in range(m_data):
        cells = np.sort(rng.choice(live, size=min(live, int(rng.integers(2, 7))), replace=False))
        fdm = rng.uniform(0.2, 1.0, len(cells))
        az = rng.uniform(0, np.pi)
        for blk, f in enumerate((1.0, np.cos(2 * az), np.sin(2 * az))[:nblk]):
            r += [row] * len(cells)
            c += list(blk * kmax * ncell + period[row] * ncell + cells)
            v += list(fdm * f)
    r, c, v = np.array(r, np.int64), np.array(c, np.int64), np.array(v, np.float32)
    if smooth > 0:
        lr, lc, lv = laplacian2d(nx, ny, np.full(nblk * kmax, smooth, np.float32))
        if no_reg_period is not None:
            keep = (lc % (kmax * ncell)) // ncell != no_reg_period
            lr, lc, lv = lr[keep], lc[keep], lv[keep]
        r, c, v = np.concatenate([r, lr + m_data]), np.concatenate([c, lc]), np.concatenate([v, lv])
        m = m_data + nblk * kmax * ncell
    else:
        m = m_data
    return dict(nx=nx, ny=ny, kmax=kmax, azim=bool(azim), damp=float(np.float32(damp)), m=m, m_data=m_data, n=nblk * kmax * ncell,
                irow=(r + 1).astype(np.int32), icol=(c + 1).astype(np.int32), rw=v, dead=ncell - 1 if ncell > 1 else None)


# ---- rows longer than one stride of the device loops (tests/test_long_rows_*.py) ----
LONG_DATA_LENS = (63, 64, 65, 127, 128, 129, 200)          # both sides of one and two strides of 64 in mp_accum_rows, and a fourth stride
LONG_REG_LENS = (7, 8, 9, 63, 64, 65, 66)                  # both sides of MP_EMAX = 8 in k_mp_rows and of a stride of 64
LONG_SHAPES = {False: (17, 16), True: (12, 9)}             # n_g = 210: one block of 210, three of 70
LONG_KMAX = 2
LONG_REG_ROWS = 257                                        # period 0 gets the list again and again up to a second batch of MP_TB = 256


def long_rows(nx, ny, kmax, azim, smooth, damp, data_lens, reg_lens, seed=0, through_dead=False):
    """`problem` with more rows, of exactly the lengths given per period (data_lens[p], reg_lens[p]): data rows behind the data rows,
    period by period (columns of one period, distinct and ascending, drawn over all blocks without the dead cell, values uniform in
    +-3 / sqrt(len)), and regularisation rows behind the regularisation rows (row i of a period inside block i mod nblk, values
    uniform in +-max(smooth, 0.3) / sqrt(len); they are there for smooth = 0 too).  through_dead: added data row i of a period holds
    the dead cell's column of block i mod nblk, which no other data row does.  Triplets 1-based, sorted by (row, column)."""
    prob = problem(nx, ny, kmax, azim, smooth, damp, seed=seed)
    rng = np.random.default_rng(seed + 1000003)
    ncell, nblk = (nx - 2) * (ny - 2), 3 if azim else 1
    kn, dead, md0 = kmax * ncell, prob["dead"], prob["m_data"]
    glob = lambda p, loc: (loc // ncell) * kn + p * ncell + loc % ncell     # (ascends with the local index blk * ncell + cell)
    live = np.flatnonzero(np.arange(nblk * ncell) % ncell != dead)
    nd = sum(len(l) for l in data_lens)
    r, c, v = prob["irow"].astype(np.int64) - 1, prob["icol"].astype(np.int64) - 1, prob["rw"]
    r = np.where(r >= md0, r + nd, r)
    rs, cs, vs = [r], [c], [v]
    row = md0
    for p in range(kmax):
        for i, ln in enumerate(data_lens[p]):
            if through_dead:
                loc = np.sort(np.append(rng.choice(live, size=ln - 1, replace=False), (i % nblk) * ncell + dead))
            else:
                loc = np.sort(rng.choice(live, size=ln, replace=False))
            rs.append(np.full(ln, row))
            cs.append(glob(p, loc))
            vs.append((rng.uniform(-3.0, 3.0, ln) / np.sqrt(ln)).astype(np.float32))
            row += 1
    row = prob["m"] + nd
    for p in range(kmax):
        for i, ln in enumerate(reg_lens[p]):
            rs.append(np.full(ln, row))
            cs.append(glob(p, (i % nblk) * ncell + np.sort(rng.choice(ncell, size=ln, replace=False))))
            vs.append((rng.uniform(-1.0, 1.0, ln) * max(smooth, 0.3) / np.sqrt(ln)).astype(np.float32))
            row += 1
    r, c, v = np.concatenate(rs), np.concatenate(cs), np.concatenate(vs)
    order = np.lexsort((c, r))
    prob.update(m=row, m_data=md0 + nd, irow=(r[order] + 1).astype(np.int32), icol=(c[order] + 1).astype(np.int32), rw=v[order])
    return prob


def long_case(azim, reg, through_dead=False):
    """the long-row problem of the tests: LONG_SHAPES at LONG_KMAX periods, six data rows of each of LONG_DATA_LENS per period;
    LONG_REG_LENS once per period, and in period 0 as often as brings its regularisation rows to LONG_REG_ROWS or more"""
    nx, ny = LONG_SHAPES[azim]
    base = (3 if azim else 1) * (nx - 2) * (ny - 2) if reg[0] > 0 else 0
    reps = [max(1, -(-(LONG_REG_ROWS - base) // len(LONG_REG_LENS)))] + [1] * (LONG_KMAX - 1)
    data = [tuple(l for l in LONG_DATA_LENS for _ in range(6))] * LONG_KMAX
    return long_rows(nx, ny, LONG_KMAX, azim, reg[0], reg[1], data, [LONG_REG_LENS * k for k in reps], seed=nx * 100 + ny + 7 * azim + LONG_KMAX,
                     through_dead=through_dead)


def groups(prob):
    """per period: D, the regularisation rows (dense, in ascending row order) in the local index blk*ncell + cell; the number of data rows"""
    nvx, nvy, kmax = prob["nx"] - 2, prob["ny"] - 2, prob["kmax"]
    ncell = nvx * nvy
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
        out.append((dense[:nd].T @ dense[:nd], dense[nd:], nd))
    return out


def derived(prob, per_period, sel):
    """the arrays of Context.map_posterior from (C, Rm) per period (None for a period that could not be factored)"""
    nvx, nvy, kmax = prob["nx"] - 2, prob["ny"] - 2, prob["kmax"]
    ncell = nvx * nvy
    nblk = 3 if prob["azim"] else 1
    ng = nblk * ncell
    out = {k: np.full((nblk, kmax, nvy, nvx), np.nan) for k in PER_UNKNOWN}
    out["trace"] = np.full((nblk, kmax), np.nan)
    out["rows"] = None if sel is None else np.full((kmax, len(sel), ng), np.nan)
    out["n_failed"] = 0
    blk = np.arange(ng) // ncell
    ci, cj = (np.arange(ng) % ncell) % nvx, (np.arange(ng) % ncell) // nvx
    for p, one in enumerate(per_period):
        if one is None:
            out["n_failed"] += 1
            continue
        C, Rm = one
        vals = dense_ref.per_unknown(C, Rm, blk, ci, cj)
        vals["width"] = vals.pop("width_h")
        for k, v in vals.items():
            out[k][:, p] = v.reshape(nblk, nvy, nvx)
        out["trace"][:, p] = np.diag(Rm).reshape(nblk, ncell).sum(axis=1)
        if sel is not None:
            out["rows"][p] = Rm[np.asarray(sel)]
    if not prob["azim"]:
        out["leak"] = None
    return out


def normal_matrix(prob, D, L):
    return D + L.T @ L + prob["damp"] ** 2 * np.eye(len(D))


def linalg(prob, sel=None):
    per = []
    for D, L, _ in groups(prob):
        A = normal_matrix(prob, D, L)
        try:
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            per.append(None)
            continue
        C = np.linalg.inv(A)
        per.append((C, C @ D))
    return derived(prob, per, sel)


def route(prob, sel=None):
    per = []
    for D, L, _ in groups(prob):
        R = dense_ref.cholesky(normal_matrix(prob, D, L))
        if R is None:
            per.append(None)
            continue
        C = dense_ref.gram_of_inverse(dense_ref.inverse_factor(R))
        Rm = np.eye(len(D))
        for l in L:                                          # the regularisation rows one by one, ascending, every row a at once
            e = np.flatnonzero(l)
            t = C[:, e] @ l[e]
            Rm[:, e] -= np.outer(t, l[e])
        Rm -= prob["damp"] ** 2 * C
        per.append((C, Rm))
    return derived(prob, per, sel)


def worst(got, ref, keys=OUTPUTS):
    return dense_ref.worst(got, ref, keys)
