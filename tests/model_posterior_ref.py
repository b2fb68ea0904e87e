"""NumPy fp64 statements of dazim_model_posterior (include/dazim.h) from COO triplets, and the problems its
tests run on.  `linalg` is the independent reference (numpy.linalg.inv of the normal matrix, Rm = C D), `route` follows the kernels
(right-looking Cholesky, M = R^-1 by forward substitution, C = M^T M, Rm = I - C P entry by entry from the regularisation rows and
the damping last).  Both return the arrays of Context.model_posterior in fp64."""
import numpy as np

from tests import dense_ref

PER_UNKNOWN = ("std_post", "std_noise", "rdiag", "rsum", "width_h", "width_z", "leak")
OUTPUTS = PER_UNKNOWN + ("trace", "rows")

NB, TS = 32, 64   # the panel width of the factorisation and the tile of the dense kernels: n below sits on both sides of either
# (nx, ny, nz) with n = ncell (nz-1) = 1, 31, 32, 33, 65, 135, 150
SHAPES_ISO = [(3, 3, 2), (33, 3, 2), (6, 6, 3), (13, 3, 4), (15, 3, 6), (11, 7, 4), (8, 7, 6)]
# n = 3 ncell (nz-1) = 3, 30, 33, 63, 66, 135, 450; (8, 7, 6) has inner cells in all three directions and seven tiles
SHAPES_JOINT = [(3, 3, 2), (7, 3, 3), (13, 3, 2), (9, 3, 4), (13, 3, 3), (7, 5, 4), (8, 7, 6)]
REGS = [(0.7, 0.3), (0.0, 0.5), (0.8, 0.0)]
REG_IDS = ["smooth+damp", "damp", "smooth"]
COND_MAX = 1e4    # cond(A_n) of every problem the GPU tests run on (asserted in tests/test_model_posterior_ref_cpu.py)


def dims(prob):
    nvx, nvy, nlay = prob["nx"] - 2, prob["ny"] - 2, prob["nz"] - 1
    nblk = 3 if prob["joint"] else 1
    return nvx, nvy, nlay, nblk, nvx * nvy, nblk * nvx * nvy * nlay


def tikhonov3d(nx, ny, nz, weights):
    """the rows of dazim_csr_append_tikhonov as 0-based (row, col, value) triplets: block b on columns b*maxvp .., weight weights[b];
    a cell on a face of the block the single entry 2w, an inner cell 6w and -w on its six neighbours; rows in block, k, j, i order"""
    nvx, nvy, nlay = nx - 2, ny - 2, nz - 1
    ncell = nvx * nvy
    maxvp = ncell * nlay
    r, c, v = [], [], []
    for b, w in enumerate(np.asarray(weights, np.float32)):
        for u in range(maxvp):
            k, cell = divmod(u, ncell)
            j, i = divmod(cell, nvx)
            row = col = b * maxvp + u
            if i in (0, nvx - 1) or j in (0, nvy - 1) or k in (0, nlay - 1):
                r.append(row); c.append(col); v.append(np.float32(2.0) * w)
            else:
                for d, f in ((-ncell, -1.0), (-nvx, -1.0), (-1, -1.0), (0, 6.0), (1, -1.0), (nvx, -1.0), (ncell, -1.0)):
                    r.append(row); c.append(col + d); v.append(np.float32(f) * w)
    return np.array(r, np.int64), np.array(c, np.int64), np.array(v, np.float32)


def problem(nx, ny, nz, joint, smooth, damp, seed=0, nray=None):
    """random ray-like data rows: 2-6 cells, every knot of them weighted by a per-row depth kernel (a bump about a random depth), with
    joint the cos / sin 2 psi copies in the Gc and Gs blocks, as a ray's row; the regularisation rows of tikhonov3d with weight
    `smooth` on every block (none for smooth = 0) and the damping.  The last cell of the map is crossed by no row (when there is more
    than one cell).  Triplets 1-based, as Context.csr_from_coo takes them; the values are fp32."""
    rng = np.random.default_rng(seed)
    nvx, nvy, nlay = nx - 2, ny - 2, nz - 1
    ncell, nblk = nvx * nvy, 3 if joint else 1
    maxvp = ncell * nlay
    live = max(ncell - 1, 1)
    m_data = nray if nray is not None else 2 * ncell * nlay + 3
    r, c, v = [], [], []
    for row in range(m_data):
        cells = np.sort(rng.choice(live, size=min(live, int(rng.integers(2, 7))), replace=False))
        fdm = rng.uniform(0.2, 1.0, len(cells))
        depth = np.exp(-((np.arange(nlay) - rng.uniform(0, nlay - 1 if nlay > 1 else 0)) / rng.uniform(0.6, 1.5)) ** 2)
        az = rng.uniform(0, np.pi)
        cols = (np.arange(nlay)[:, None] * ncell + cells[None, :]).reshape(-1)
        vals = (depth[:, None] * fdm[None, :]).reshape(-1)
        for blk, f in enumerate((1.0, np.cos(2 * az), np.sin(2 * az))[:nblk]):
            r += [row] * len(cols)
            c += list(blk * maxvp + cols)
            v += list(vals * f)
    r, c, v = np.array(r, np.int64), np.array(c, np.int64), np.array(v, np.float32)
    if smooth > 0:
        lr, lc, lv = tikhonov3d(nx, ny, nz, np.full(nblk, smooth, np.float32))
        r, c, v = np.concatenate([r, lr + m_data]), np.concatenate([c, lc]), np.concatenate([v, lv])
        m = m_data + nblk * maxvp
    else:
        m = m_data
    return dict(nx=nx, ny=ny, nz=nz, joint=bool(joint), damp=float(np.float32(damp)), m=m, m_data=m_data, n=nblk * maxvp,
                depz=(4.0 * np.arange(nlay) ** 1.3).astype(np.float32), irow=(r + 1).astype(np.int32), icol=(c + 1).astype(np.int32), rw=v,
                dead=ncell - 1 if ncell > 1 else None)


# ---- rows longer than one pass of the device loops (tests/test_long_rows_*.py) ----
# both sides of one and two passes of mo_accum_row (64 * MO_UN = 256 entries a pass), and 300: a second pass with padding lanes
LONG_LENS = (255, 256, 257, 300, 511, 512, 513)
LONG_REG_SHORT = (7, 8, 9, 63, 64, 65)
LONG_SHAPES = {False: (13, 12, 6), True: (10, 9, 6)}       # iso n = 550, one block; joint n = 840, blocks of 280
LONG_DATA = tuple(l for l in LONG_LENS for _ in range(12))
LONG_REG = {False: tuple(l for l in LONG_LENS for _ in range(2)) + LONG_REG_SHORT,
            True: tuple(l for l in LONG_LENS if l <= 257 for _ in range(2)) + LONG_REG_SHORT}


def long_rows(nx, ny, nz, joint, smooth, damp, data_lens, reg_lens, seed=0):
    """`problem` with more rows, of exactly the lengths given: data rows behind the data rows (columns distinct and ascending, drawn
    over all blocks without the dead cell, values uniform in +-3 / sqrt(len)), and regularisation rows behind the regularisation rows
    (row i inside block i mod nblk, values uniform in +-max(smooth, 0.3) / sqrt(len); they are there for smooth = 0 too).  Every added
    data row holds the column prob["hub"]: the live column most of `problem`'s data rows hold, so that one column of the transpose is
    long as well.  The added rows do not depend on smooth and damp but for that factor.  Triplets 1-based, sorted by (row, column)."""
    prob = problem(nx, ny, nz, joint, smooth, damp, seed=seed)
    rng = np.random.default_rng(seed + 1000003)
    nvx, nvy, nlay, nblk, ncell, n = dims(prob)
    maxvp = ncell * nlay
    md0 = prob["m_data"]
    r, c, v = prob["irow"].astype(np.int64) - 1, prob["icol"].astype(np.int64) - 1, prob["rw"]
    live = np.flatnonzero(np.arange(n) % ncell != prob["dead"])
    hub = int(np.argmax(np.bincount(c[r < md0], minlength=n)))
    rest = live[live != hub]
    r = np.where(r >= md0, r + len(data_lens), r)
    rs, cs, vs = [r], [c], [v]
    for i, ln in enumerate(data_lens):
        rs.append(np.full(ln, md0 + i))
        cs.append(np.sort(np.append(rng.choice(rest, size=ln - 1, replace=False), hub)))
        vs.append((rng.uniform(-3.0, 3.0, ln) / np.sqrt(ln)).astype(np.float32))
    m = prob["m"] + len(data_lens)
    for i, ln in enumerate(reg_lens):
        rs.append(np.full(ln, m + i))
        cs.append((i % nblk) * maxvp + np.sort(rng.choice(maxvp, size=ln, replace=False)))
        vs.append((rng.uniform(-1.0, 1.0, ln) * max(smooth, 0.3) / np.sqrt(ln)).astype(np.float32))
    r, c, v = np.concatenate(rs), np.concatenate(cs), np.concatenate(vs)
    order = np.lexsort((c, r))
    prob.update(m=m + len(reg_lens), m_data=md0 + len(data_lens), hub=hub, irow=(r[order] + 1).astype(np.int32),
                icol=(c[order] + 1).astype(np.int32), rw=v[order])
    return prob


def long_case(joint, reg):
    """the long-row problem of the tests: LONG_SHAPES, twelve data rows of each of LONG_LENS, LONG_REG"""
    nx, ny, nz = LONG_SHAPES[joint]
    return long_rows(nx, ny, nz, joint, reg[0], reg[1], LONG_DATA, LONG_REG[joint], seed=nx * 10000 + ny * 100 + nz + 7 * joint)


def truncated(prob, keep, reg_only=False):
    """the problem without the entries behind the first `keep` of every row (reg_only: of every regularisation row): what a row
    walk that stops after `keep` entries would see"""
    row = prob["irow"].astype(np.int64) - 1
    first = np.searchsorted(row, row, side="left")            # (the triplets are sorted by row)
    on = (np.arange(len(row)) - first < keep) | ((row < prob["m_data"]) if reg_only else False)
    return dict(prob, irow=prob["irow"][on], icol=prob["icol"][on], rw=prob["rw"][on])


def row_lengths(prob):
    """(lengths of the data rows, lengths of the regularisation rows)"""
    ln = np.bincount(prob["irow"].astype(np.int64) - 1, minlength=prob["m"])
    return ln[:prob["m_data"]], ln[prob["m_data"]:]


def parts(prob):
    """D = sum of r^T r over the data rows, and the regularisation rows (dense, in ascending row order)"""
    n = dims(prob)[5]
    row, col, val = prob["irow"].astype(np.int64) - 1, prob["icol"].astype(np.int64) - 1, prob["rw"].astype(np.float64)
    dense = np.zeros((prob["m"], n))
    np.add.at(dense, (row, col), val)
    nd = prob["m_data"]
    return dense[:nd].T @ dense[:nd], dense[nd:]


def normal_matrix(prob, D, L):
    return D + L.T @ L + prob["damp"] ** 2 * np.eye(len(D))


def derived(prob, one, sel):
    """the arrays of Context.model_posterior from (C, Rm) (None: the matrix could not be factored)"""
    nvx, nvy, nlay, nblk, ncell, n = dims(prob)
    maxvp = ncell * nlay
    shape = (nblk, nlay, nvy, nvx)
    out = {k: np.full(shape, np.nan) for k in PER_UNKNOWN}
    out["trace"] = np.full((nblk, nlay), np.nan)
    out["rows"] = None if sel is None else np.full((len(sel), n), np.nan)
    out["n_failed"] = 1 if one is None else 0
    if one is not None:
        C, Rm = one
        a = np.arange(n)
        blk, k, cell = a // maxvp, (a % maxvp) // ncell, a % ncell
        for key, val in dense_ref.per_unknown(C, Rm, blk, cell % nvx, cell // nvx, prob["depz"].astype(np.float64)[k]).items():
            out[key] = val.reshape(shape)
        out["trace"] = np.diag(Rm).reshape(nblk, nlay, ncell).sum(axis=2)
        if sel is not None:
            out["rows"] = Rm[np.asarray(sel)]
    if not prob["joint"]:
        out["leak"] = None
    return out


def linalg(prob, sel=None):
    D, L = parts(prob)
    A = normal_matrix(prob, D, L)
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return derived(prob, None, sel)
    C = np.linalg.inv(A)
    return derived(prob, (C, C @ D), sel)


def route(prob, sel=None):
    D, L = parts(prob)
    n = len(D)
    R = dense_ref.cholesky(normal_matrix(prob, D, L))
    if R is None:
        return derived(prob, None, sel)
    C = dense_ref.gram_of_inverse(dense_ref.inverse_factor(R))
    T = C @ L.T                                          # t_l of every unknown a: T[a, l] = sum_e C_ae l_e
    Rm = np.eye(n)
    for c in range(n):                                   # the gather: column c's regularisation entries, ascending rows
        for l in np.flatnonzero(L[:, c]):
            Rm[:, c] -= T[:, l] * L[l, c]
    Rm -= prob["damp"] ** 2 * C
    return derived(prob, (C, Rm), sel)


def worst(got, ref, keys=OUTPUTS):
    return dense_ref.worst(got, ref, keys)
