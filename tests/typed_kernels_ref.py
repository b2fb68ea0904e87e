"""The reference's depthkernel (inv/CalSurfG.f90:1-139) for one (iwave, igr), composed of pieces that exist: the oracle's Brocher
relations and refineGrid2LayerMdl (orc_brocher, orc_refine_layers) and a surfdisp96 with every argument that the caller passes in --
Oracle.surfdisp96_full (the C restatement), Ref.surfdisp96_full (the reference subroutine itself) or Context.surfdisp96 (the device,
`batched`: all models of a segment in one call).  The yardstick of dazim_dispersion_kernels_typed, and the common model its tests share.

depthkernel's arithmetic outside surfdisp96, restated here in fp32 / fp64 as the reference rounds it:
  perturbed knot  b0 -+ (0.5 * dln) * b0 in fp32, dln = 0.01 (:77,:83); variants in the order knot, (vs, vp, rho), (-, +)
  kernel          (cg2 - cg1) / dble(dln * b0), the fp32 product widened (:92), cg the fp32-rounded curves in fp64
and two definitions of dazim_dispersion_kernels_typed (include/dazim.h) on top of it:
  the depth kernels of an entry whose own curve has ended (pv = 0) are 0;
  the Vp kernel of a Love segment is 0 (`love_vp_zero`).  The SH period equation (dltar1) does not read Vp; the subroutine's only
  use of it for a Love wave is the start value of the first period's search (gtsolh of the slowest layer, inv/surfdisp96.f:361),
  so the reference's own Love Vp "kernel" is the trace of two searches that start 0.5 % apart and stop within nevill's tolerance
  |c1 - c2| <= 1e-6 c1 (:608) of the same root: noise.  tests/test_typed_kernels_ref_cpu.py measures it (love_vp_zero=False) and
  holds it to that tolerance."""
import ctypes as C

import numpy as np

f32 = np.float32

# ---- the common model of tests/test_disp_typed_gpu.py, test_typed_kernels_ref_cpu.py, test_typed_G_gpu.py ----
NX, NY = 5, 4
DEPZ = np.array([0, 5, 12, 22, 35], f32)
SUBLAYERS = 3.0
RC, RG, LC, LG = (2, 0), (2, 1), (1, 0), (1, 1)
SEGMENTS = [RC + (np.array([6.0, 12.0, 20.0]),), RG + (np.array([6.0, 12.0, 20.0]),), LC + (np.array([6.0, 12.0, 20.0]),),
            LG + (np.array([8.0, 16.0]),)]
# columns (= iy * NX + ix): uniform Vs / a slow second knot / Vs falling with depth
COL_UNIFORM, COL_LVZ, COL_FALLING = 7, 13, 16
SEED = 2024


def common_model(nx=NX, ny=NY, seed=SEED, ended=True):
    """vel [nz][ny][nx] fp32: Vs rising with depth, a seeded +-4 % scatter per knot.  Column COL_LVZ has a slow second knot.
    Column COL_UNIFORM has one Vs at every knot: the Earth flattening turns that into a gradient of 0.5 % over these 35 km, which
    carries a Love wave at the short periods and none at 20 s -- its Love phase curve ends at the third period (the search leaves
    its window as in tests/test_surfdisp_full_gpu.py::test_halfspace_has_no_love_wave).  Column COL_FALLING has Vs falling by 1 % per
    knot: the subroutine still finds sign changes of the SH period equation at the short periods, and its Love phase curve ends at
    the third period, its Love group curve at the second.  tests/test_typed_kernels_ref_cpu.py pins where these curves end.
    ended=False leaves those two columns as drawn (every curve complete: maps that an eikonal solver can take)."""
    rng = np.random.default_rng(seed)
    prof = np.array([3.0, 3.3, 3.6, 3.9, 4.3])
    vel = prof[:, None] * (1.0 + 0.04 * rng.uniform(-1.0, 1.0, (len(prof), nx * ny)))
    if ended:
        vel[:, COL_UNIFORM] = 3.4
        vel[:, COL_FALLING] = 3.4 * 0.99 ** np.arange(len(prof))
    vel[1, COL_LVZ] = 0.85 * vel[0, COL_LVZ]
    return np.ascontiguousarray(vel.reshape(len(prof), ny, nx), f32)


def offsets(segments):
    """first virtual period of every segment, and K"""
    off = np.concatenate([[0], np.cumsum([len(s[2]) for s in segments])]).astype(int)
    return off[:-1], int(off[-1])


def _oracle():
    from oracle.pyoracle import Oracle
    o = Oracle()
    o.lib.orc_refine_layers.restype = C.c_int
    return o


def column_stacks(vsz, depz, sublayers, orc=None, perturbed=True):
    """the 1 + 6 nz layer stacks depthkernel hands to surfdisp96 for one column: (thk, vp, vs, rho) [1 + 6 nz][nlayer] fp32, and
    the unperturbed knots (vs, vp, rho) [3][nz]; without `perturbed` the column's own stack alone"""
    from oracle.pyoracle import pf
    o = orc or _oracle()
    depz = np.ascontiguousarray(depz, f32)
    vsz = np.ascontiguousarray(vsz, f32)
    nz = len(vsz)
    vpz, rhoz = np.zeros(nz, f32), np.zeros(nz, f32)
    for k in range(nz):
        vp, rho = C.c_float(0), C.c_float(0)
        o.lib.orc_brocher(C.c_float(float(vsz[k])), C.byref(vp), C.byref(rho))
        vpz[k], rhoz[k] = vp.value, rho.value
    knots = np.stack([vsz, vpz, rhoz])

    def refine(kn):
        out = [np.zeros(200, f32) for _ in range(4)]
        n = o.lib.orc_refine_layers(C.c_float(sublayers), nz, pf(depz), pf(np.ascontiguousarray(kn[1])), pf(np.ascontiguousarray(kn[0])),
                                    pf(np.ascontiguousarray(kn[2])), *(pf(x) for x in out))
        return [x[:n].copy() for x in out]

    stacks = [refine(knots)]
    half_dln = f32(0.5) * f32(0.01)
    for i in range(nz if perturbed else 0):
        for q in range(3):
            for sign in (-1, 1):
                kn = knots.copy()
                b0 = knots[q, i]
                kn[q, i] = b0 - half_dln * b0 if sign < 0 else b0 + half_dln * b0
                stacks.append(refine(kn))
    return [np.stack([s[j] for s in stacks]) for j in range(4)], knots


def depthkernel_typed(vel, depz, sublayers, iwave, igr, periods, sd, batched=False, kernels=True, love_vp_zero=True):
    """depthkernel with (iwave, igr), mode 1, iflsph 1: pv [kmax][ncol], (sen_vs, sen_vp, sen_rho) [nz][kmax][ncol] fp64.
    sd(thk, vp, vs, rho, t, iflsph, iwave, mode, igr) -> cg (or (cg, n_failed)); batched: called once with [nmodel][nlayer] arrays"""
    o = _oracle()
    nz = vel.shape[0]
    cols = np.ascontiguousarray(vel, f32).reshape(nz, -1).T
    ncol, kmax, nvar = len(cols), len(periods), 1 + 6 * nz
    t = np.ascontiguousarray(periods, np.float64)
    if not kernels:
        nvar = 1
    per_col = [column_stacks(c, depz, sublayers, o, perturbed=kernels) for c in cols]
    stacks = [np.concatenate([p[0][j] for p in per_col]) for j in range(4)]     # [ncol * nvar][nlayer]
    if batched:
        cg = sd(*stacks, t, 1, iwave, 1, igr)
        cg = cg[0] if isinstance(cg, tuple) else cg
    else:
        cg = np.stack([sd(*(s[m] for s in stacks), t, 1, iwave, 1, igr) for m in range(len(stacks[0]))])
    cg = np.asarray(cg, np.float64).reshape(ncol, nvar, kmax)
    pv = np.ascontiguousarray(cg[:, 0, :].T)
    if not kernels:
        return pv, None
    sen = [np.zeros((nz, kmax, ncol), np.float64) for _ in range(3)]
    for col in range(ncol):
        knots = per_col[col][1]
        for i in range(nz):
            for q in range(3):
                cg1, cg2 = cg[col, 1 + 6 * i + 2 * q], cg[col, 2 + 6 * i + 2 * q]
                den = np.float64(f32(0.01) * knots[q, i])
                if not (love_vp_zero and iwave == 1 and q == 1):
                    sen[q][i, :, col] = np.where(cg[col, 0] != 0, (cg2 - cg1) / den, 0.0)
    return pv, sen


def typed_tables(vel, depz, sublayers, segments, sd, batched=False, kernels=True):
    """the tables of dazim_dispersion_kernels_typed from depthkernel_typed, segment after segment: pv [K][ncol], sen 3 x [nz][K][ncol]
    (None without `kernels`: the curves alone, one model per column)"""
    parts = [depthkernel_typed(vel, depz, sublayers, iw, ig, t, sd, batched, kernels) for iw, ig, t in segments]
    pv = np.concatenate([p[0] for p in parts], axis=0)
    sen = [np.concatenate([p[1][q] for p in parts], axis=1) for q in range(3)] if kernels else None
    return pv, sen


def brocher_knots(vel):
    """(vs, vp, rho) [3][nz][ncol] fp32 of every column: the `base` of the kernels' denominators"""
    o = _oracle()
    nz = vel.shape[0]
    cols = np.ascontiguousarray(vel, f32).reshape(nz, -1)
    out = np.zeros((3,) + cols.shape, f32)
    out[0] = cols
    for idx in np.ndindex(cols.shape):
        vp, rho = C.c_float(0), C.c_float(0)
        o.lib.orc_brocher(C.c_float(float(cols[idx])), C.byref(vp), C.byref(rho))
        out[1][idx], out[2][idx] = vp.value, rho.value
    return out


def check_tables(name, got, want, vel, segments, pool=None):
    """got = (pv, sen) against want = (pv, sen) under the bars tests/test_surfdisp_full_gpu.py states for a device (or another libm)
    against the reference, segment by segment:
      phase velocity  |d| <= one fp32 ulp of c (C_ULP), bit-equal on >= C_SHARE of the entries
      group velocity  |d| <= U_ABS on the entries that are not bit-equal, bit-equal on >= U_SHARE
      a curve ends at the same period
    and, pushed through the quotient (cg2 - cg1) / (0.01 base), two values each within its bar:
      kernels         |d| <= 2 bar / (0.01 base) entry by entry (base = the knot's Vs, Vp or rho), bit-equal on >= 1 - 2 (1 - share):
                      an entry is exempt only if one of its two curves is.
    got[1] / want[1] None (a curves-only call): pv alone.
    pool: a dict -- the per-entry bars are asserted here, the bit-equal shares are not: the counts [equal, entries] are added to
    pool[(iwave, igr, table)] for check_pooled_shares, which holds them to the same shares over several models (a model with a few
    dozen entries cannot express a 1 % allowance)."""
    from tests.bars import at_least, within
    from tests.test_surfdisp_full_gpu import C_SHARE, C_ULP, U_ABS, U_SHARE
    base = brocher_knots(vel)
    off, K = offsets(segments)

    def shares(what, table, g, w, bar):
        if pool is None:
            at_least(f"{what} bit-equal share", (g == w).mean(), bar)
        else:
            print(f"\n[measured] {what} bit-equal share: {(g == w).mean():.6f} ({int((g == w).sum())} of {g.size}, pooled)")
            cnt = pool.setdefault(table, [0, 0])
            cnt[0] += int((g == w).sum())
            cnt[1] += g.size

    assert (got[1] is None) == (want[1] is None)
    for (iw, ig, t), o in zip(segments, off):
        sl = slice(o, o + len(t))
        tag = f"{name} iwave={iw} igr={ig}"
        bar, share = (U_ABS, U_SHARE) if ig else (C_ULP, C_SHARE)
        g, w = got[0][sl], want[0][sl]
        assert np.array_equal(g == 0, w == 0), f"{tag}: curves end at different periods"
        within(f"{tag} pv max |d| km/s", np.abs(g - w).max(), bar)
        shares(f"{tag} pv", (iw, ig, "pv"), g, w, share)
        if got[1] is None:
            continue
        for q, qn in enumerate(("sen_vs", "sen_vp", "sen_rho")):
            g, w = got[1][q][:, sl], want[1][q][:, sl]
            qbar = 2.0 * bar / (np.float64(0.01) * base[q].astype(np.float64))[:, None, :]
            ratio = (np.abs(g - w) / qbar).max()
            within(f"{tag} {qn} max |d| / (2 bar / (0.01 base))", ratio, 1.0)
            shares(f"{tag} {qn}", (iw, ig, qn), g, w, 1.0 - 2.0 * (1.0 - share))


def check_pooled_shares(name, pool):
    """the bit-equal shares of check_tables on the counts that its `pool` collected, per wave type and table"""
    from tests.bars import at_least
    from tests.test_surfdisp_full_gpu import C_SHARE, U_SHARE
    for (iw, ig, table), (equal, n) in sorted(pool.items()):
        share = U_SHARE if ig else C_SHARE
        at_least(f"{name} iwave={iw} igr={ig} {table} bit-equal share of {n} pooled entries", equal / n,
                 share if table == "pv" else 1.0 - 2.0 * (1.0 - share))
