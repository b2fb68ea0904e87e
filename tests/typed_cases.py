"""Inputs shared by tests/test_typed_cases_cpu.py and tests/test_disp_typed_shapes_gpu.py: models at which the host code of
dazim_dispersion_kernels_typed (dazimsurftomo_amd/csrc/disp_typed.hip) splits its work and lays out its LDS tables in another way
than on the common model of tests/typed_kernels_ref.py (64 items and 5 columns per workgroup, a patch of 8 layers, 17 layers),
and `plan`, a restatement of that host arithmetic in Python (no GPU import).

A case is dict(depz, sublayers, nx, ny, segments, kernels, vel[nz][ny][nx] fp32, falling): `falling` is the column whose Vs falls
with depth (None: the case has none).  What each case reaches (mmax layers, patch rows, items `tw` and columns `cpb` per workgroup):

  two_knots      [0, 30] km: the last knot's range is interval 1 plus the half-space (the whole stack); 9 variants of a Love column,
                 so a wavefront spans 8 columns (cpb 9)
  max_knots      64 knots (NZMAX), sublayers 2: 190 of NL = 200 layers; 385 / 257 variants, so a column spans 5 to 7 workgroups and a
                 workgroup holds the tail of one column and the head of the next; 13 / 9 / 9 workgroups, 2 items in each last one
  patch_tw32     3 knots, sublayers 60: 123 layers, a patch of 122 -> 32 items per workgroup (lanes 32 .. 63 idle); the last
                 workgroups hold 31 / 1 / 1 items
  patch_tw16     2 knots, sublayers 150: 152 layers, the patch is the whole stack -> 16 items
  curves_tw32    curves only (cpb = tw + 1 base tables): 16 knots / 61 layers -> 32 items, 3 workgroups with 6 items in the last
  curves_tw16    curves only, 30 knots / 117 layers -> 16 items
  curves_tw8     curves only, 50 knots / 197 layers -> 8 items, 4 in the last workgroup
  curves_tw64_last, curves_tw32_first
                 curves only on 2 knots: the largest number of layers for which the host's loop still keeps 64 items, and one
                 layer more (32 items).  The two sublayer counts are taken from `plan` (boundary_sublayers), not written down
  one_column     the common knots, one column: col0 + c >= ncol on every base table of the workgroup but the first
  np60           the common knots, Rayleigh and Love group only, 60 periods each (NP)

Unless a case says otherwise its segments are Rayleigh group and Love phase at 6, 12, 20 s and Love group at 8, 16 s -- no
Rayleigh-phase segment, which would go to dazim_dispersion_kernels -- and its velocities are linspace(3.0, 4.4, nz) with a seeded
+-3 % scatter per knot and column."""
import types

import numpy as np

from tests import typed_kernels_ref as T

f32 = np.float32
NL, NP, NZMAX, TW, LDS_MAX = 200, 60, 64, 64, 64 * 1024       # the constants of disp_typed.hip

T3, T2 = np.array([6.0, 12.0, 20.0]), np.array([8.0, 16.0])
SEGMENTS = [T.RG + (T3,), T.LC + (T3,), T.LG + (T2,)]
SEGMENTS_NP60 = [T.RG + (np.linspace(3.0, 90.0, NP),), T.LG + (np.linspace(3.0, 90.0, NP),)]
SEED = 2025


# ---- the host's plan ----
def refine_layers(depz, sublayers):
    """dz_refine_layers (csrc/dazim_internal.h) in its fp32 expressions: the interval (1-based) of every refined layer, 0 for the
    half-space that ends the table"""
    depz, s = np.asarray(depz, f32), f32(sublayers)
    iv = []
    for i in range(1, len(depz)):
        thk = f32(depz[i] - depz[i - 1])
        minthk = f32(thk / s)
        nsub = int(f32(f32(thk + f32(1.0e-4)) / minthk)) + 1
        iv += [i] * nsub
    return np.array(iv + [0])


def plan(depz, sublayers, segments, kernels, ncol):
    """What the host of dazim_dispersion_kernels_typed decides for a call: mmax layers, npatch rows of the patch table, and for the
    segments that typed_kernel runs (all but Rayleigh phase, in call order: `typed`, their indices in `segments`) the variants per
    column nvar[], the workgroups blocks[] with blk0[] the first of each, the items last[] of each segment's last workgroup; tw items
    and cpb columns per workgroup and the bytes of LDS they take.  tw = 0: no plan fits (the host refuses)."""
    nz = len(depz)
    iv = refine_layers(depz, sublayers)
    mmax = len(iv)
    krange = np.zeros((nz + 1, 2), int)          # per knot: first layer (1-based) and number of layers it touches
    for pi in range(1, nz + 1):
        hit = np.flatnonzero(((iv == pi - 1) & (pi > 1)) | (iv == pi) | ((iv == 0) & (pi == nz)))
        if len(hit):
            krange[pi] = hit[0] + 1, hit[-1] - hit[0] + 1
    npatch = int(krange[:, 1].max()) if kernels else 0
    typed = [s for s, (iw, ig, _) in enumerate(segments) if (iw, ig) != T.RC]
    nvar = [1 + (4 if segments[s][0] == 1 else 6) * nz if kernels else 1 for s in typed]
    nvar_min = min(nvar)
    tw, cpb, lds = TW, 0, 0
    while tw >= 1:
        cpb = (tw + nvar_min - 1) // nvar_min + 1
        lds = (8 * mmax + 4 * cpb * mmax + 3 * npatch * tw + 3 * cpb * nz) * 4
        if lds <= LDS_MAX:
            break
        tw //= 2
    blocks = [(ncol * v + tw - 1) // tw for v in nvar] if tw else []
    last = [ncol * v - (b - 1) * tw for v, b in zip(nvar, blocks)]
    blk0 = [int(x) for x in np.concatenate([[0], np.cumsum(blocks)])]
    return types.SimpleNamespace(nz=nz, ncol=ncol, mmax=mmax, npatch=npatch, krange=krange, typed=typed, nvar=nvar, tw=tw, cpb=cpb,
                                 lds=lds, blocks=blocks, blk0=blk0, last=last)


def columns_of_workgroups(p, g):
    """[(first column, last column)] of every workgroup of typed segment g: the columns its items belong to"""
    nwork = p.ncol * p.nvar[g]
    return [(b * p.tw // p.nvar[g], (min((b + 1) * p.tw, nwork) - 1) // p.nvar[g]) for b in range(p.blocks[g])]


def workgroups_of_column(p, g, col):
    """(first, last) workgroup of typed segment g that holds variants of column `col`"""
    return col * p.nvar[g] // p.tw, ((col + 1) * p.nvar[g] - 1) // p.tw


def boundary_sublayers(depz=(0.0, 40.0), ncol=70):
    """the largest sublayer count (an integer) of a curves-only call on `depz` for which the host keeps 64 items per workgroup, from
    `plan`: (sublayers, mmax) of it and of the next count up"""
    s = 1
    while plan(depz, float(s + 1), SEGMENTS, False, ncol).tw == TW:
        s += 1
    return [(float(x), plan(depz, float(x), SEGMENTS, False, ncol).mmax) for x in (s, s + 1)]


# ---- the cases ----
def falling_profile(nz):
    """Vs falling by 4 % over the knots: the column whose Love curves end (tests/typed_kernels_ref.py: COL_FALLING is this on 5 knots)"""
    return 3.4 * 0.99 ** np.linspace(0.0, 4.0, nz)


def _case(depz, sublayers, nx, ny, kernels=True, segments=SEGMENTS, falling=None, seed=SEED):
    depz = np.asarray(depz, f32)
    nz = len(depz)
    rng = np.random.default_rng(seed + nz)
    vel = np.linspace(3.0, 4.4, nz)[:, None] * (1.0 + 0.03 * rng.uniform(-1.0, 1.0, (nz, nx * ny)))
    if falling is not None:
        vel[:, falling] = falling_profile(nz)
    vel = np.ascontiguousarray(vel.reshape(nz, ny, nx), f32)
    vel.setflags(write=False)
    return dict(depz=depz, sublayers=float(sublayers), nx=nx, ny=ny, segments=segments, kernels=kernels, vel=vel, falling=falling)


def cases():
    """{name: case}, in a fixed order.  The falling columns: where the variants of one column lie in two workgroups of the Love
    segments (two_knots: column 7 = items 63 .. 71; patch_tw32: column 4 = items 52 .. 64, its last variant alone in the last
    workgroup; patch_tw16: column 1 = items 9 .. 17); a curves-only call has one item per column, so there the column is the first
    item of the last, partial workgroup (column 64 of 70)."""
    out = {}
    out["two_knots"] = _case([0.0, 30.0], 3.0, 4, 2, falling=7)
    out["max_knots"] = _case(2.0 * np.arange(NZMAX), 2.0, 2, 1)
    out["patch_tw32"] = _case([0.0, 20.0, 45.0], 60.0, 5, 1, falling=4)
    out["patch_tw16"] = _case([0.0, 40.0], 150.0, 3, 1, falling=1)
    out["curves_tw32"] = _case(3.0 * np.arange(16), 3.0, 10, 7, kernels=False, falling=64)
    out["curves_tw16"] = _case(3.0 * np.arange(30), 3.0, 10, 7, kernels=False)
    out["curves_tw8"] = _case(3.0 * np.arange(50), 3.0, 5, 4, kernels=False)
    (s64, _), (s32, _) = boundary_sublayers()
    out["curves_tw64_last"] = _case([0.0, 40.0], s64, 10, 7, kernels=False, falling=64)
    out["curves_tw32_first"] = _case([0.0, 40.0], s32, 10, 7, kernels=False, falling=64)
    out["one_column"] = _case(T.DEPZ, T.SUBLAYERS, 1, 1, falling=0)
    out["np60"] = _case(T.DEPZ, T.SUBLAYERS, 3, 1, segments=SEGMENTS_NP60)
    return out


def case_plan(c):
    return plan(c["depz"], c["sublayers"], c["segments"], c["kernels"], c["nx"] * c["ny"])


# what `plan` must give (the issue's table, worked out from the host code by hand): mmax, npatch, tw, cpb
EXPECTED = {
    "two_knots": (5, 5, 64, 9), "max_knots": (190, 6, 64, 2), "patch_tw32": (123, 122, 32, 4), "patch_tw16": (152, 152, 16, 3),
    "curves_tw32": (61, 0, 32, 33), "curves_tw16": (117, 0, 16, 17), "curves_tw8": (197, 0, 8, 9), "one_column": (17, 8, 64, 5),
    "np60": (17, 8, 64, 5),
}
# (blocks, items of the last workgroup) per typed segment, where the issue states them
EXPECTED_BLOCKS = {
    "max_knots": ([13, 9, 9], [2, 2, 2]), "patch_tw32": ([3, 3, 3], [31, 1, 1]), "curves_tw32": ([3, 3, 3], [6, 6, 6]),
    "curves_tw8": ([3, 3, 3], [4, 4, 4]),
}
# the Love curves of these cases' falling columns end (tests/test_typed_cases_cpu.py pins where); in the deep models none does
FALLING_ENDS = ("two_knots", "patch_tw32", "patch_tw16", "curves_tw32", "curves_tw64_last", "curves_tw32_first", "one_column")


def tables(c, sd, batched=False):
    """the yardstick of a case: typed_kernels_ref.typed_tables driven by the surfdisp96 `sd`, curves only where the case is"""
    return T.typed_tables(c["vel"], c["depz"], c["sublayers"], c["segments"], sd, batched=batched, kernels=c["kernels"])
