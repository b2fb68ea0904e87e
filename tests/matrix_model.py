"""A NumPy model of the resident matrix (dazim_csr) for tests/test_matrix_lifecycle_gpu.py: the COO triplets in fp32, rows ascending
and columns ascending inside a row (the order dazim_csr_to_coo returns), and every mutation of the library mirrored on them.  The
row generators are vectorised (the large shapes append 120 000 rows); tests/test_matrix_model_cpu.py pins them to the loops
`tikhonov_coo` (tests/test_outer_iteration_gpu.py) and `lap2d_numpy` (tests/test_phase_maps_gpu.py) follow."""
import numpy as np

f32 = np.float32


def tikhonov_rows(nx, ny, nz, weights, row_lo=0, row_hi=None):
    """rows [row_lo, row_hi) of TikhRegul_joint's len(weights) * maxvp rows (inv/TikhRegul.f90:107-209): (row - row_lo, column,
    value), 0-based, ascending columns.  A cell on a face of its block: 2w; an interior cell: 6w and six times -w."""
    nvx, nvz, nzm1 = nx - 2, ny - 2, nz - 1
    maxvp = nvx * nvz * nzm1
    w = np.asarray(weights, f32)
    if row_hi is None:
        row_hi = maxvp * len(w)
    R = np.arange(row_lo, row_hi, dtype=np.int64)
    blk, cell = R // maxvp, R % maxvp
    k, rem = cell // (nvx * nvz), cell % (nvx * nvz)
    j, i = rem // nvx, rem % nvx
    face = (i == 0) | (i == nvx - 1) | (j == 0) | (j == nvz - 1) | (k == 0) | (k == nzm1 - 1)
    cnt = np.where(face, 1, 7)
    rows = np.repeat(R - row_lo, cnt)
    first = np.cumsum(cnt) - cnt                                   # first entry of each row
    q = np.arange(len(rows)) - np.repeat(first, cnt)               # position inside the row
    fe = np.repeat(face, cnt)
    d = np.array([-nvz * nvx, -nvx, -1, 0, 1, nvx, nvz * nvx], np.int64)
    cols = np.repeat(blk * maxvp + cell, cnt) + np.where(fe, 0, d[q])
    we = np.repeat(w[blk], cnt).astype(f32)
    coef = np.where(fe, f32(2.0), np.where(q == 3, f32(6.0), f32(-1.0))).astype(f32)
    return rows, cols, (coef * we).astype(f32)


def laplacian2d_rows(nx, ny, weights):
    """dazim_csr_append_laplacian2d's len(weights) * (nx-2)(ny-2) rows: an edge cell 2w, an inner cell 4w and four times -w"""
    nvx, nvz = nx - 2, ny - 2
    ncell = nvx * nvz
    w = np.asarray(weights, f32)
    R = np.arange(ncell * len(w), dtype=np.int64)
    b, cell = R // ncell, R % ncell
    j, i = cell // nvx, cell % nvx
    edge = (i == 0) | (i == nvx - 1) | (j == 0) | (j == nvz - 1)
    cnt = np.where(edge, 1, 5)
    rows = np.repeat(R, cnt)
    first = np.cumsum(cnt) - cnt
    q = np.arange(len(rows)) - np.repeat(first, cnt)
    ee = np.repeat(edge, cnt)
    d = np.array([-nvx, -1, 0, 1, nvx], np.int64)
    cols = np.repeat(R, cnt) + np.where(ee, 0, d[q])
    we = np.repeat(w[b], cnt).astype(f32)
    coef = np.where(ee, f32(2.0), np.where(q == 2, f32(4.0), f32(-1.0))).astype(f32)
    return rows, cols, (coef * we).astype(f32)


class Model:
    """m x n matrix as 0-based triplets (rows, cols int64; vals fp32) in canonical order"""

    def __init__(self, m, n, rows, cols, vals):
        self.m, self.n = int(m), int(n)
        self.rows, self.cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        self.vals = np.asarray(vals, f32)
        assert self.vals.dtype == f32 and len(self.rows) == len(self.cols) == len(self.vals)
        key = self.rows * self.n + self.cols
        assert (np.diff(key) > 0).all(), "canonical order, no duplicate (row, col)"

    @property
    def nnz(self):
        return len(self.vals)

    def copy(self):
        return Model(self.m, self.n, self.rows.copy(), self.cols.copy(), self.vals.copy())

    def coo(self):
        """1-based int32 triplets, what csr_from_coo takes and to_coo returns"""
        return (self.rows + 1).astype(np.int32), (self.cols + 1).astype(np.int32), self.vals.copy()

    def csr64(self):
        """the matrix in fp64 (scipy CSR, straight from the canonical order)"""
        import scipy.sparse as sp
        indptr = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=self.m))])
        return sp.csr_matrix((self.vals.astype(np.float64), self.cols, indptr), shape=(self.m, self.n))

    def append(self, extra_m, rows, cols, vals):
        """rows given relative to the first appended row"""
        self.rows = np.concatenate([self.rows, np.asarray(rows, np.int64) + self.m])
        self.cols = np.concatenate([self.cols, np.asarray(cols, np.int64)])
        self.vals = np.concatenate([self.vals, np.asarray(vals, f32)])
        self.m += int(extra_m)

    def append_tikhonov_rows(self, nx, ny, nz, weights, row_lo=0, row_hi=None):
        if row_hi is None:
            row_hi = (nx - 2) * (ny - 2) * (nz - 1) * len(weights)
        self.append(row_hi - row_lo, *tikhonov_rows(nx, ny, nz, weights, row_lo, row_hi))

    def append_laplacian2d(self, nx, ny, weights):
        self.append((nx - 2) * (ny - 2) * len(weights), *laplacian2d_rows(nx, ny, weights))

    def scale_rows(self, w, nrows=None):
        """rw(i) = rw(i) * w(row(i)) for the rows below nrows (inv/Main_Jt.f90:467-469), one fp32 product per entry"""
        w = np.asarray(w, f32)
        nrows = self.m if nrows is None else nrows
        sel = self.rows < nrows
        self.vals[sel] = (self.vals[sel] * w[self.rows[sel]]).astype(f32)

    def threshold(self, tol):
        keep = np.abs(self.vals) > f32(tol)
        return Model(self.m, self.n, self.rows[keep], self.cols[keep], self.vals[keep])
