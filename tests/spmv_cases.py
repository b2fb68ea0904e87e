"""Integer-valued sparse matrices for tests/test_spmv_exact_gpu.py, and a NumPy model of how the library dispatches and walks them
(no GPU import; tests/test_spmv_cases_cpu.py checks this module on its own).

Values in {+-1..+-7} and vectors in {+-1..+-8}, stored as fp32, with sum |v||x| < 2^24 per row and sum |v||y| < 2^24 per column:
every fp32 partial sum of A x, in any lane assignment or combine order, and every 64-bit fixed-point sum of A^T y is an exactly
representable integer, so each kernel form must return the bits of an int64 product.  A dropped, doubled or misplaced entry moves
a result by at least 1.

A case is built from C = the device's compute-unit count (the dispatch thresholds are multiples of it): an empty first row, a
block of planted rows, vectorised filler rows, a few duplicate (row, column) pairs and -- except where the case says otherwise --
a tail of rows shorter than 64 entries.  A planted row lies in ONE column block and starts at a chosen CSR position mod 4 (a
spacer row of one to three entries in front of it moves the position), so that its (row, block) segment, its (row, block pair)
segment and the row itself are the same entry range; `missing_classes` counts the planted classes back from the built matrix.

`rows` in CASES counts the filler rows: the planted rows and the tail come on top (m is a few hundred larger)."""
import functools

import numpy as np
import scipy.sparse as sp

f32 = np.float32

# the dispatch thresholds of sparse.hip, restated: LDSX_MAX floats of x fit the LDS; the blocked and scatter forms want 2^22 entries
# and 16 rows per compute unit, the whole-x LDS form 64; rows of >= 64 entries are "long"; 16 lanes per segment serve long rows
# averaging fewer than 600 entries per block pair (A x) or 400 per block (A^T y)
LDSX_MAX = 38 * 1024
NNZ_MIN = 1 << 22
ROWS_WALK, ROWS_LDSX = 16, 64
SPLIT_SHORT = 64
AVG_AX, AVG_ATY = 600.0, 400.0
LDSX_LENGTHS = (256, 512, 768, 1024, 1792, 2048, 2600)

# n, ncb (column blocks of the scatter form: the library reports its cut as spmv.ncb / spmv.cbw), filler rows(C), filler entries
# per row lo..hi, tail: "short" rows of 0..63 entries | "last64" one row of exactly 64 entries last | None (no row reaches 64)
CASES = {
    "long64":        dict(n=19453, ncb=1, rows=lambda C: 16 * C + 37, fill=(1020, 1060), tail="short"),
    "long64_last64": dict(n=19453, ncb=1, rows=lambda C: 16 * C + 37, fill=(1020, 1060), tail="last64"),
    "ldsx":          dict(n=19453, ncb=1, rows=lambda C: 64 * C + 5, fill=(258, 280), tail="short"),
    "allshort":      dict(n=19453, ncb=1, rows=lambda C: max(70001, 64 * C + 1), fill=(59, 63), tail=None),
    "blk64":         dict(n=40003, ncb=3, rows=lambda C: 16 * C + 3, fill=(1240, 1290), tail="short"),
    "blk16":         dict(n=40003, ncb=3, rows=lambda C: 32 * C + 8, fill=(514, 540), tail="short"),
    "pairlocal":     dict(n=70001, ncb=4, rows=lambda C: 16 * C + 1, fill=(1390, 1430), tail="short"),
}
# what each case must select: A x kind (0 plain, 1 whole x in LDS, 2 column-blocked), lanes, index bytes; the same for A^T y
# (kind 1 scatter); whether the matrix splits into long rows and a short tail
EXPECT = {
    "long64":        dict(spmv_kind=0, spmv_lanes=0, spmv_idx=4, spmvt_kind=1, spmvt_lanes=64, spmvt_idx=2, split=True),
    "long64_last64": dict(spmv_kind=0, spmv_lanes=0, spmv_idx=4, spmvt_kind=1, spmvt_lanes=64, spmvt_idx=2, split=False),
    "ldsx":          dict(spmv_kind=1, spmv_lanes=0, spmv_idx=2, spmvt_kind=1, spmvt_lanes=16, spmvt_idx=2, split=True),
    "allshort":      dict(spmv_kind=1, spmv_lanes=0, spmv_idx=2, spmvt_kind=1, spmvt_lanes=16, spmvt_idx=2, split=False),
    "blk64":         dict(spmv_kind=2, spmv_lanes=64, spmv_idx=2, spmvt_kind=1, spmvt_lanes=64, spmvt_idx=2, split=True),
    "blk16":         dict(spmv_kind=2, spmv_lanes=16, spmv_idx=2, spmvt_kind=1, spmvt_lanes=16, spmvt_idx=2, split=True),
    "pairlocal":     dict(spmv_kind=2, spmv_lanes=64, spmv_idx=2, spmvt_kind=1, spmvt_lanes=16, spmvt_idx=2, split=True),
}


def block_width(n, ncb):
    return ((n + ncb - 1) // ncb + 3) & ~3


class Case:
    """irow, icol (1-based int32, shuffled), rw fp32; x, y, x0, y0 integer-valued fp32 vectors; marks: planted row ids (0-based)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @functools.cached_property
    def S(self):
        """the matrix in int64 (duplicates summed)"""
        return sp.csr_matrix((self.rw.astype(np.int64), (self.irow.astype(np.int64) - 1, self.icol.astype(np.int64) - 1)),
                             shape=(self.m, self.n))

    @functools.cached_property
    def order(self):
        """the canonical order (rows ascending, columns ascending inside a row, equal pairs in the caller's order)"""
        key = (self.irow.astype(np.int64) - 1) * self.n + (self.icol.astype(np.int64) - 1)
        return np.argsort(key, kind="stable")

    @functools.cached_property
    def csr(self):
        """rowptr [m + 1], 0-based columns in canonical order"""
        lens = np.bincount(self.irow.astype(np.int64) - 1, minlength=self.m)
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), self.icol[self.order].astype(np.int64) - 1

    @functools.cached_property
    def refs(self):
        """int64 products: A x, A^T y, sum |v| per column"""
        xi, yi = self.x.astype(np.int64), self.y.astype(np.int64)
        return dict(Ax=self.S @ xi, ATy=self.S.T @ yi, colabs=np.asarray(abs(self.S_abs).sum(axis=0)).ravel())

    @functools.cached_property
    def S_abs(self):
        """|v| entry by entry (duplicates summed after the absolute value, as the kernels see them)"""
        return sp.csr_matrix((np.abs(self.rw).astype(np.int64), (self.irow.astype(np.int64) - 1, self.icol.astype(np.int64) - 1)),
                             shape=(self.m, self.n))

    def bounds(self):
        """the largest sum |v||x| over the rows (with |y0| on top) and sum |v||y| over the columns (with |x0|): both must stay
        below 2^24 for the int64 reference to be what exact fp32 arithmetic gives"""
        ax = self.S_abs @ np.abs(self.x).astype(np.int64) + np.abs(self.y0).astype(np.int64)
        aty = self.S_abs.T @ np.abs(self.y).astype(np.int64) + np.abs(self.x0).astype(np.int64)
        return int(ax.max()), int(aty.max())


class _Rows:
    """triplets in any order plus the length of every row in row order: `pos` is where the next row starts in the CSR arrays"""

    def __init__(self, n, ncb, cbw, rng):
        self.n, self.ncb, self.cbw, self.rng = n, ncb, cbw, rng
        self.lens, self.rows, self.cols, self.pos = [], [], [], 0

    @property
    def m(self):
        return len(self.lens)

    def block(self, b):
        return b * self.cbw, min((b + 1) * self.cbw, self.n)

    def add(self, cols):
        cols = np.asarray(cols, np.int64)
        self.rows.append(np.full(len(cols), self.m, np.int64)); self.cols.append(cols)
        self.lens.append(len(cols)); self.pos += len(cols)
        return self.m - 1

    def in_block(self, L, b):
        lo, hi = self.block(b)
        return lo + self.rng.choice(hi - lo, L, replace=False)

    def plant(self, a, L, b=None):
        """a row of L entries in column block b whose first entry sits at a CSR position = a mod 4 (None: anywhere)"""
        if b is None:
            b = int(self.rng.integers(0, self.ncb))
        if a is not None and self.pos % 4 != a:
            self.add(self.in_block((a - self.pos) % 4, int(self.rng.integers(0, self.ncb))))   # the spacer
        return self.add(self.in_block(L, b))

    def filler(self, count, lo, hi):
        """count rows of lo..hi distinct columns: a random start and cumulative steps, mod n (the columns wrap over the blocks)"""
        rng, n = self.rng, self.n
        lens = rng.integers(lo, hi + 1, count)
        steps = rng.integers(1, (n - 1) // hi + 1, (count, hi), dtype=np.int32)
        cols = (rng.integers(0, n, count, dtype=np.int32)[:, None] + np.cumsum(steps, axis=1, dtype=np.int32)) % n
        keep = np.arange(hi)[None, :] < lens[:, None]
        first = self.m
        self.rows.append(np.repeat(np.arange(first, first + count, dtype=np.int64), lens)); self.cols.append(cols[keep].astype(np.int64))
        # duplicate (row, column) pairs, one of them three times, in rows that stay within hi entries
        room = np.flatnonzero(lens < hi - 1)
        dup = rng.choice(room, min(48, len(room)), replace=False)
        dup = np.concatenate([dup, dup[:1]])
        self.rows.append(first + dup); self.cols.append(cols[dup, 0].astype(np.int64))
        self.dup_chunk = len(self.cols) - 1
        self.orig = sum(len(c) for c in self.cols[:-2]) + (np.cumsum(lens) - lens)[dup]   # where the repeated entries are
        lens = lens + np.bincount(dup, minlength=count)
        self.lens.extend(lens.tolist()); self.pos += int(lens.sum())
        return first + dup


def boundary_columns(n, ncb, cbw):
    return sorted({0, n - 1} | {b * cbw - 1 for b in range(1, ncb)} | {b * cbw for b in range(1, ncb)})


def _plant_short(R):
    """what every walk can reach: each length 0..7 at each start alignment, each (start, end) alignment among segments of 8..11
    entries, a row in each block alone, the block-boundary columns"""
    for a in range(4):
        for L in range(8):
            R.plant(a, L)
    for a in range(4):
        for em in range(4):
            R.plant(a, 8 + (em - a) % 4)
    for b in range(R.ncb):
        R.plant(None, 40, b)
    return R.add(boundary_columns(R.n, R.ncb, R.cbw))


@functools.lru_cache(maxsize=2)
def build(name, C):
    cfg = CASES[name]
    n, ncb = cfg["n"], cfg["ncb"]
    cbw = block_width(n, ncb)
    rng = np.random.default_rng(sorted(CASES).index(name) + 1000)
    R = _Rows(n, ncb, cbw, rng)
    marks = {}
    R.add([])                                                     # an empty first row
    marks["boundary"] = _plant_short(R)
    if cfg["tail"] is not None:                                   # rows of 64 entries and more are allowed
        for K in (4 * 16 * 2, 4 * 64 * 4):                        # 4 * GL * NG entries are prefetched: the long-row loop starts behind them
            for A in (K - 4, K, K + 4, 2 * K + 8):
                R.plant(0, A)
                R.plant(1, 3 + A + 2)                             # a head of three and a tail of two around the same aligned part
        if ncb == 1:
            for T in LDSX_LENGTHS:
                for L in (T - 1, T, T + 1):
                    R.plant(None, L, 0)
        marks["wide"] = R.add(np.unique(np.concatenate([boundary_columns(n, ncb, cbw), rng.choice(n, 300, replace=False)])))
    marks["dups"] = R.filler(cfg["rows"](C), *cfg["fill"])
    if cfg["tail"] == "short":
        marks["tail"] = R.plant(None, 7, 0)                      # the first row of the tail is not empty
        _plant_short(R)
        R.plant(None, 63)
        for L in rng.integers(0, 64, 60):
            R.add(rng.choice(n, int(L), replace=False))           # ... over all blocks
        R.add([])                                                 # the matrix ends in empty rows ...
        while R.m % 4 == 0 or (R.m - marks["tail"]) % 4 == 0:     # ... and neither row count is a multiple of 4 (at most two more)
            R.add([])
    elif cfg["tail"] == "last64":
        marks["last"] = R.plant(None, 64, 0)
    m = R.m
    rows, cols = np.concatenate(R.rows), np.concatenate(R.cols)
    nnz = len(rows)
    vals = rng.integers(1, 8, nnz) * rng.choice([-1, 1], nnz)
    # the duplicates are the last triplets (the tail holds none): their values differ from the entry they repeat and, for the
    # pair that is there three times, from each other
    ndup = len(marks["dups"])
    tail_len = nnz - sum(len(c) for c in R.cols[:R.dup_chunk + 1])
    vals[R.orig] = 2
    vals[nnz - tail_len - ndup:nnz - tail_len] = np.where(np.arange(ndup) % 2 == 0, -5, 3)
    vals[nnz - tail_len - 1] = 7
    perm = rng.permutation(nnz)

    def vec(k):
        return (rng.integers(1, 9, k) * rng.choice([-1, 1], k)).astype(f32)
    return Case(name=name, C=C, m=m, n=n, nnz=nnz, ncb=ncb, cbw=cbw, lens=np.asarray(R.lens, np.int64), marks=marks,
                irow=(rows[perm] + 1).astype(np.int32), icol=(cols[perm] + 1).astype(np.int32), rw=vals[perm].astype(f32),
                x=vec(n), y=vec(m), x0=vec(n), y0=vec(m))


# ---- the model of the dispatch and of walk_rows' alignment ----

def split_rows(lens):
    """dazim_csr::split_row and long_avg: 1 + the last row of >= 64 entries and the mean length of the rows in front of it; a
    matrix without such a row, or with it last, does not split"""
    m = len(lens)
    long_rows = np.flatnonzero(lens >= SPLIT_SHORT)
    last = int(long_rows[-1]) + 1 if len(long_rows) else 0
    if 0 < last < m:
        return last, float(lens[:last].sum()) / last
    return m, float(lens.sum()) / m


def dispatch(case, C, split=True):
    """what the library's statistics must report after A x and A^T y on this matrix (default options; split: spmv.split)"""
    m, n, nnz, ncb = case.m, case.n, case.nnz, case.ncb
    walk = nnz >= NNZ_MIN and m >= ROWS_WALK * C
    blocked = walk and n > LDSX_MAX
    ldsx = n <= LDSX_MAX and m >= ROWS_LDSX * C
    mod16 = 0 if n <= 65536 else 2 * case.cbw
    col16 = mod16 <= 65536
    srow, avg = split_rows(case.lens)
    if not split:
        srow, avg = m, float(nnz) / m
    npair = (ncb + 1) // 2
    return dict(spmv_kind=2 if blocked else (1 if ldsx else 0),
                spmv_lanes=(16 if avg < AVG_AX * npair else 64) if blocked else 0,
                spmv_idx=2 if col16 and (blocked or (ldsx and mod16 == 0)) else 4,
                spmvt_kind=1 if walk else 0,
                spmvt_lanes=(16 if avg < AVG_ATY * ncb else 64) if walk else 0,
                spmvt_idx=2 if col16 and walk else 4,
                split_row=srow)


def segments(case, pairs=False):
    """s, e [m, nseg]: the entry range of every (row, column block) segment, or (row, pair of column blocks) segment"""
    rowptr, col = case.csr
    W = case.ncb * case.cbw + 1
    key = np.repeat(np.arange(case.m, dtype=np.int64), np.diff(rowptr)) * W + col
    cuts = np.arange(case.ncb + 1, dtype=np.int64) * case.cbw
    cb = np.searchsorted(key, np.arange(case.m, dtype=np.int64)[:, None] * W + cuts[None, :])
    assert np.array_equal(cb[:, 0], rowptr[:-1]) and np.array_equal(cb[:, -1], rowptr[1:])
    if pairs:
        idx = list(range(0, case.ncb, 2)) + [case.ncb]
        cb = cb[:, idx]
    return cb[:, :-1], cb[:, 1:]


def walk_parts(s, e):
    """walk_rows' cut of a segment: head (<= 3 entries up to the next multiple of four, clipped at e), aligned groups of four, tail"""
    s4 = np.minimum((s + 3) & ~3, e)
    e4 = s4 + ((e - s4) & ~3)
    return s4 - s, e4 - s4, e - e4


def _walk_classes(s, e, K, where, miss):
    s, e = s.ravel(), e.ravel()
    L = e - s
    short = set(zip(L[L < 8].tolist(), (s[L < 8] % 4).tolist()))
    miss += [f"{where}: length {l} at start {a} mod 4" for l in range(8) for a in range(4) if (l, a) not in short]
    ends = set(zip((s[L >= 8] % 4).tolist(), (e[L >= 8] % 4).tolist()))
    miss += [f"{where}: start {a} end {b} mod 4" for a in range(4) for b in range(4) if (a, b) not in ends]
    head, al, tail = walk_parts(s, e)
    assert np.all(head + al + tail == L) and np.all(head <= 3) and np.all(tail <= 3) and np.all(al % 4 == 0)
    if K:
        for A in (K - 4, K, K + 4):
            for h, t in ((0, 0), (3, 2)):
                if not np.any((al == A) & (head == h) & (tail == t)):
                    miss.append(f"{where}: aligned part {A}, head {h}, tail {t}")
        if not np.any(al > 2 * K):
            miss.append(f"{where}: aligned part > {2 * K}")


def missing_classes(case, C):
    """the planted classes that the built matrix does NOT hold (empty: all present), counted from its canonical CSR arrays"""
    miss = []
    d = dispatch(case, C)
    rowptr, col = case.csr
    lens = np.diff(rowptr)
    assert np.array_equal(lens, case.lens)
    srow, m = d["split_row"], case.m
    reach_long = CASES[case.name]["tail"] is not None             # rows of >= 64 entries exist
    walks = [("A^T y", d["spmvt_lanes"], segments(case))]
    if d["spmv_kind"] == 2:
        walks.append(("A x", d["spmv_lanes"], segments(case, pairs=True)))
    for tag, lanes, (s, e) in walks:
        K = 4 * lanes * (4 if lanes == 64 else 2)
        _walk_classes(s[:srow], e[:srow], K if reach_long else 0, f"{tag}, long rows, {lanes} lanes", miss)
        if srow < m:
            _walk_classes(s[srow:], e[srow:], 0, f"{tag}, short tail", miss)
    if d["spmv_kind"] == 1 and reach_long:
        have = set(lens.tolist())
        miss += [f"row of {L} entries" for T in LDSX_LENGTHS for L in (T - 1, T, T + 1) if L not in have]
    # columns
    rows_of = np.repeat(np.arange(m), lens)
    for c in boundary_columns(case.n, case.ncb, case.cbw):
        r = rows_of[col == c]
        if not np.any(r < srow) or (srow < m and not np.any(r >= srow)):
            miss.append(f"column {c} in the long rows and in the tail")
    s, e = segments(case)
    for b in range(case.ncb):
        alone = (e[:, b] - s[:, b] == lens) & (lens > 0)
        if not np.any(alone[:srow]) or (srow < m and not np.any(alone[srow:])):
            miss.append(f"a row in column block {b} alone")
    if lens[0] != 0:
        miss.append("an empty first row")
    if not np.any(lens[1:srow - 1] == 0):
        miss.append("an empty row among the long rows")
    if CASES[case.name]["tail"] == "short":
        t = lens[srow:]
        if srow == m or len(t) % 4 == 0 or m % 4 == 0 or not np.any(t == 0) or t[0] == 0 or t.max() != 63 or lens[srow - 1] < 64:
            miss.append("a tail of short rows, some empty, the first not, their count no multiple of 4")
        if srow < m and case.refs["Ax"][srow] == 0:
            miss.append("a non-zero product in the first row of the tail")
    if CASES[case.name]["tail"] == "last64" and (lens[-1] != 64 or srow != m):
        miss.append("a last row of exactly 64 entries")
    if CASES[case.name]["tail"] is None and lens.max() >= 64:
        miss.append("no row of 64 entries")
    dup = np.flatnonzero((np.diff(col) == 0) & (np.diff(rows_of) == 0))
    if len(dup) < 8 or not np.any(np.diff(dup) == 1):
        miss.append("duplicate (row, column) pairs, one three times")
    return miss
