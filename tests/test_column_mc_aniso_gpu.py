"""-m gpu: Gc/Gs posteriors from the Monte-Carlo Vs chains (dazim_mc_set_aniso / _aniso_step / _aniso_state / _aniso_result, DESIGN.md
section 14).

The sample against its NumPy restatement (tests/mc_aniso_ref.py) at the shapes where the kernel can go wrong, the identity with
dazim_column_lsq, the chain left bit for bit alone, dazim_mc_run against the hand-made loop, recovery with the real forward model
and the refused calls."""
import time

import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_aniso_ref as ref

pytestmark = pytest.mark.gpu

# fp64 sums against numpy.linalg: max |device - reference| / max |reference| per array.  Measured over the 20 cases of
# test_step_against_numpy: asum 1.1e-16 .. 2.3e-15 below nlay 63 and 8.8e-14 .. 1.57e-13 at nlay 63, kmax 60; avar 6.7e-17 ..
# 2.3e-15 and 1.9e-14 .. 2.9e-14.  The bar is twice the largest.  (The fp32 results were equal, 0 ulp, in every case.)
SUM_BAR = 3.2e-13


@pytest.fixture(scope="module")
def ctx():
    dz.build()
    c = dz.Context(0)
    yield c
    c.close()


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def assert_one_ulp(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), what
    d = ulps(a[~nan], b[~nan])
    # (+0 and -0 are the same number)
    d[(a[~nan] == 0) & (b[~nan] == 0)] = 0
    assert d.size == 0 or d.max() <= 1, (what, int(d.max()))


def trend_kernels(rng, nlay, kmax, ncol):
    """random Lsen_Gsc-like tables [nlay][kmax][ncol]: a ridge that deepens with the period, 20 % scatter per entry"""
    dep = np.arange(nlay)[:, None, None]
    per = np.arange(kmax)[None, :, None]
    centre = per * max(nlay - 1, 1) / max(kmax - 1, 1)
    base = 0.03 * np.exp(-0.5 * ((dep - centre) / (1.0 + 0.15 * nlay)) ** 2)
    return (base * (1 + 0.2 * rng.random((nlay, kmax, ncol))) * (1 + 0.3 * rng.random((1, 1, ncol)))).astype(np.float32)


def grid_problem(ctx, rng, nlay, kmax, nchain, ntemp, proposal=0, seed=21, nadapt=3):
    """5 x 5 nodes: 9 inner cells, the middle one without Vs data (so cs != cell behind it), cell (0, 2) with wa all 0"""
    nx = ny = 5
    nz = nlay + 1
    sh = (ny - 2, nx - 2)
    vel0 = rng.uniform(3.0, 4.5, (nz, ny, nx)).astype(np.float32)
    vmin = rng.uniform(2.8, 3.4, (nlay,) + sh).astype(np.float32)
    vmax = (vmin + rng.uniform(0.3, 1.2, vmin.shape)).astype(np.float32)
    cobs = rng.uniform(3.2, 4.0, (kmax,) + sh).astype(np.float32)
    wdat = rng.uniform(50, 150, (kmax,) + sh).astype(np.float32)
    wdat[:, 1, 1] = 0.0
    mc = ctx.mc_create(nx, ny, nz, kmax, nchain, 16, seed, vel0, vmin, vmax, cobs, wdat, 0.05, nadapt, proposal=proposal,
                       ntemp=ntemp, tmax=4.0, nswap=2)
    cells = np.nonzero((wdat.reshape(kmax, -1) != 0).any(axis=0))[0]
    assert mc.n_empty == 1 and len(cells) == 8 and cells[4] == 5
    amap = rng.normal(0, 0.02, (2, kmax) + sh).astype(np.float32)
    wa = rng.uniform(300, 700, (kmax,) + sh).astype(np.float32)
    if kmax > 2:
        wa[1] = 0.0                               # a period without 2-psi data everywhere
    wa[:, 0, 2] = 0.0
    return mc, cells, cobs, amap, wa


def curves(rng, mc, cells, cobs, dead):
    """random curves near the data for every chain; the columns `dead` have no root"""
    cb = np.repeat(cobs.reshape(mc.kmax, -1)[:, cells], mc.nchain, axis=1).astype(np.float64)
    pv = (cb + rng.normal(0, 0.012, cb.shape)).astype(np.float32).astype(np.float64)
    pv[:, dead] = 0.0
    return pv


@pytest.mark.parametrize("nlay,kmax", [(1, 1), (2, 3), (5, 8), (63, 60)])
@pytest.mark.parametrize("nchain,ntemp", [(1, 1), (8, 1), (8, 4), (64, 1), (64, 4)])
def test_step_against_numpy(ctx, nlay, kmax, nchain, ntemp):
    """three samples between ordinary steps; replica group 0 of sampled cell 3 never has a root, so its rung-0 chain stays at
    chi^2 = +inf (no swap can reach it: the whole group is there) and is skipped and counted every time"""
    rng = np.random.default_rng(1000 * nlay + 10 * nchain + ntemp)
    mc, cells, cobs, amap, wa = grid_problem(ctx, rng, nlay, kmax, nchain, ntemp)
    ncold = nchain // ntemp
    ncolc = mc.ncs * ncold
    dead = 3 * nchain + np.arange(ntemp)
    lsens = [trend_kernels(rng, nlay, kmax, ncolc) for _ in range(3)]
    wK = np.stack(lsens).astype(np.float64) * wa.reshape(kmax, -1).max(axis=1)[None, None, :, None]
    nrm = np.sqrt((wK ** 2).sum(axis=2)).max()
    smooth, damp = 0.12 * nrm, 0.03 * nrm        # smooth >= a tenth of the largest column norm of diag(w) K
    mc.set_aniso(1, amap, wa, smooth, damp)
    st0 = mc.aniso_state()
    assert st0["nthin"] == 1 and st0["asum"].shape == (5, nlay, ncolc) and not st0["asum"].any() and st0["skipped"] == 0
    exp = ref.new_state(nlay, ncolc)
    cell_of_col = np.repeat(cells, ncold)
    a2, w2 = amap.reshape(2, kmax, -1), wa.reshape(kmax, -1)
    plan = [1, 1, 2]                              # ordinary steps before each sample
    for i, nstep in enumerate(plan):
        for _ in range(nstep):
            mc.step(curves(rng, mc, cells, cobs, dead), 0)
        chi2 = mc.state()["chi2"].reshape(mc.ncs, nchain)[:, ::ntemp].reshape(-1)
        assert np.isinf(chi2[3 * ncold]) and np.isinf(chi2).sum() == 1
        mc.aniso_step(lsens[i])
        ref.step(exp, lsens[i], chi2, cell_of_col, a2, w2, smooth, damp)
    got = mc.aniso_state()
    assert np.array_equal(got["acnt"], exp["acnt"]) and got["skipped"] == exp["skipped"] == 3
    rel = {}
    for k in ("asum", "avar"):
        rel[k] = float(np.abs(got[k] - exp[k]).max() / np.abs(exp[k]).max())
    print(f"\n[measured] nlay {nlay} kmax {kmax} nchain {nchain} ntemp {ntemp}: sums rel asum {rel['asum']:.2e} avar {rel['avar']:.2e}")
    assert rel["asum"] <= SUM_BAR and rel["avar"] <= SUM_BAR, rel
    # wa all 0 at cell (0, 2), sampled cell 2: x^ = 0 exactly, C the prior's
    cs0 = int(np.nonzero(cells == 2)[0][0])
    assert not got["asum"][:, :, cs0 * ncold:(cs0 + 1) * ncold].any()
    r = mc.aniso_result()
    e = ref.result(exp, cells, mc.ncell, ncold)
    assert np.array_equal(r["nsamp"].reshape(-1), e["nsamp"])
    for k in ("mean", "std", "std_between", "cov_cs"):
        a, b = r[k].reshape(e[k].shape), e[k]
        fin = ~np.isnan(b)
        d = ulps(np.ascontiguousarray(a[fin]), np.ascontiguousarray(b[fin]))
        d[(a[fin] == 0) & (b[fin] == 0)] = 0
        print(f"[measured]   {k}: max {int(d.max()) if d.size else 0} ulp")
    for k in ("mean", "std", "std_between", "cov_cs"):
        assert_one_ulp(r[k], e[k], k)
    # the cell without Vs data
    assert not r["mean"][:, :, 1, 1].any() and not r["std"][:, :, 1, 1].any() and r["nsamp"][1, 1] == 0
    if nchain == 1:                               # sampled cell 3 = cell (1, 0) has only the skipped chain: n = 0
        assert r["nsamp"][1, 0] == 0 and np.isnan(r["std"][:, :, 1, 0]).all() and not r["mean"][:, :, 1, 0].any()
    mc.free()


def test_identity_with_column_lsq(ctx):
    """the same K in every cold column of a cell: the mean is dazim_column_lsq's solution, and nothing lies between the samples"""
    rng = np.random.default_rng(8)
    nlay, kmax, nchain, ntemp = 7, 9, 8, 2
    mc, cells, cobs, amap, wa = grid_problem(ctx, rng, nlay, kmax, nchain, ntemp)
    ncold = nchain // ntemp
    Kc = trend_kernels(rng, nlay, kmax, mc.ncell)                       # per inner cell
    lsen = np.ascontiguousarray(np.repeat(Kc[:, :, cells], ncold, axis=2))
    nx = ny = 5
    table = np.zeros((nlay, kmax, ny, nx), np.float32)
    table[:, :, 1:-1, 1:-1] = Kc.reshape(nlay, kmax, ny - 2, nx - 2)
    nrm = np.sqrt(((Kc.astype(np.float64) * wa.reshape(kmax, -1).max(axis=1)[None, :, None]) ** 2).sum(axis=1)).max()
    smooth, damp = np.float32(0.12 * nrm), np.float32(0.03 * nrm)
    mc.set_aniso(1, amap, wa, smooth, damp)
    for _ in range(3):
        mc.step(curves(rng, mc, cells, cobs, []), 0)
        mc.aniso_step(lsen)
    r = mc.aniso_result()
    x, ne, _ = ctx.column_lsq(nx, ny, nlay, table.reshape(nlay, kmax, ny * nx), amap, wa, smooth, damp)
    assert ne == 1                                # cell (0, 2), where wa is all 0
    sampled = np.zeros((ny - 2, nx - 2), bool).reshape(-1)
    sampled[cells] = True
    sampled = sampled.reshape(ny - 2, nx - 2)
    assert (r["nsamp"][sampled] == 3 * ncold).all()
    assert_one_ulp(r["mean"][:, :, sampled], x[:, :, sampled], "mean against column_lsq")
    q = np.float32(2.0 ** -23)
    assert (r["std_between"][:, :, sampled] <= q * np.abs(r["mean"][:, :, sampled])).all()
    assert (np.abs(r["cov_cs"][:, sampled]) <= q * np.abs(r["mean"][0][:, sampled] * r["mean"][1][:, sampled])).all()
    assert (r["std"][:, :, sampled] > 0).all()
    mc.free()


def test_chain_not_disturbed(ctx):
    """kind 1, ntemp 4, one seed: with Gc/Gs on and samples interleaved the Vs side returns the same bytes as without"""
    out = []
    for aniso in (False, True):
        rng = np.random.default_rng(31)
        nlay, kmax, nchain, ntemp = 4, 6, 16, 4
        mc, cells, cobs, amap, wa = grid_problem(ctx, rng, nlay, kmax, nchain, ntemp, proposal=1)
        lsen = trend_kernels(rng, nlay, kmax, mc.ncs * (nchain // ntemp))
        if aniso:
            mc.set_aniso(2, amap, wa, 1.0, 0.2)
        for t in range(36):
            mc.step(curves(rng, mc, cells, cobs, []), int(t >= 26))
            if aniso and t % 3 == 1:
                mc.aniso_step(lsen)
        st, cv, tp, rs = mc.state(), mc.cov_state(), mc.temper_state(), mc.result()
        assert cv["cov_set"].any() and tp["swap_acc"].sum() > 0
        if aniso:
            assert mc.aniso_state()["acnt"].min() == 12
        out.append({**{"st." + k: v for k, v in st.items()}, **{"cv." + k: v for k, v in cv.items()},
                    **{"tp." + k: v for k, v in tp.items()}, **{"rs." + k: v for k, v in rs.items()}})
        mc.free()
    for k in out[0]:
        assert np.asarray(out[0][k]).tobytes() == np.asarray(out[1][k]).tobytes(), k


def disp_problem(ctx, nx, ny, seed, ntemp, proposal, sigma_c=0.01):
    depz = np.array([0.0, 8.0, 20.0, 35.0, 60.0], np.float32)
    periods = np.array([6.0, 8.0, 10.0, 14.0, 18.0, 24.0, 30.0, 40.0])
    nz, kmax = len(depz), len(periods)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    truth = np.zeros((nz, ny, nx), np.float32)
    for k, z in enumerate(depz):
        truth[k] = 2.9 + 0.025 * z + 0.12 * np.sin(0.9 * ii + 0.5 * k) * np.cos(0.7 * jj)
    pv, _, nf = ctx.depthkernel(truth, depz, periods, 3.0, kernels=False)
    assert nf == 0
    lsen = ctx.ti_kernels(truth, depz, periods, 3.0, pv)               # [nlay][kmax][ny*nx] at the true Vs
    sh = (ny - 2, nx - 2)
    cobs = pv.reshape(kmax, ny, nx)[:, 1:-1, 1:-1].astype(np.float32)
    mean = truth[:-1].mean(axis=(1, 2))
    vmin = np.broadcast_to((mean - 0.5)[:, None, None], (nz - 1,) + sh).astype(np.float32)
    vmax = np.broadcast_to((mean + 0.5)[:, None, None], (nz - 1,) + sh).astype(np.float32)
    wdat = np.full((kmax,) + sh, 1.0 / sigma_c, np.float32)
    # Gc/L, Gs/L smooth in depth and across the map, and their exact 2-psi terms at the true Vs
    kk = np.arange(nz - 1)[:, None, None]
    g = np.stack([0.02 * np.cos(0.6 * kk) * (1 + 0.3 * np.sin(0.8 * ii[1:-1, 1:-1])[None]),
                  0.015 * np.sin(0.5 * kk + 0.4) * (1 + 0.3 * np.cos(0.6 * jj[1:-1, 1:-1])[None])])      # [2][nlay][ny-2][nx-2]
    Kin = lsen.reshape(nz - 1, kmax, ny, nx)[:, :, 1:-1, 1:-1].astype(np.float64)
    amap = np.einsum("lpji,rlji->rpji", Kin, g).astype(np.float32)
    mc = ctx.mc_create(nx, ny, nz, kmax, 16, 100, seed, truth, vmin, vmax, cobs, wdat, proposal=proposal, ntemp=ntemp, tmax=4.0,
                       nswap=2)
    return mc, truth, depz, periods, lsen, amap, Kin


def cold(a, ncs, nchain, ntemp):
    """[n][ncol] -> the rung-0 columns [n][ncolc]"""
    return np.ascontiguousarray(a.reshape(a.shape[0], ncs, nchain)[:, :, ::ntemp].reshape(a.shape[0], -1))


@pytest.mark.parametrize("ntemp", [1, 4])
def test_run_is_the_hand_made_loop(ctx, ntemp):
    """6 x 6 cells, 4 sampled knots, 8 periods, 16 chains, nthin 5, 20 + 20 steps: dazim_mc_run against dispersion_kernels -> mc_step
    per step and, on every fifth recorded step, state -> cold columns -> dispersion_kernels -> ti_kernels -> aniso_step; then the
    run again with the pass forced into blocks of 5 cells (36 = 7 x 5 + 1)"""
    nx = ny = 8
    res = []
    for mode in ("run", "loop", "blocks"):
        mc, truth, depz, periods, lsen, amap, Kin = disp_problem(ctx, nx, ny, 6, ntemp, 0)
        nz, kmax = mc.nz, mc.kmax
        wa = np.full((kmax, ny - 2, nx - 2), 500.0, np.float32)
        mc.set_aniso(5, amap, wa, 2.0, 0.5)
        ctx.set_option("mc.aniso_block_cells", 5 if mode == "blocks" else 0)
        if mode != "loop":
            mc.run(depz, 3.0, periods, 20, 20)
            assert ctx.stat("mc.aniso_passes") == 4 and ctx.stat("mc.aniso") > 0 and ctx.stat("mc.aniso_skipped") == 0
        else:
            nrec = 0
            for t in range(40):
                prop = mc.proposals().cpu().numpy()
                pv, _, _ = ctx.depthkernel(prop.reshape(nz, 1, mc.ncol), depz, periods, 3.0, kernels=False)
                mc.step(pv, int(t >= 20))
                if t >= 20:
                    nrec += 1
                    if nrec % 5 == 0:
                        cc = cold(mc.state()["cur"], mc.ncs, mc.nchain, ntemp).reshape(nz, 1, -1)
                        pvc, _, _ = ctx.depthkernel(cc, depz, periods, 3.0, kernels=False)
                        mc.aniso_step(ctx.ti_kernels(cc, depz, periods, 3.0, pvc))
        ctx.set_option("mc.aniso_block_cells", 0)
        st, r, vs = mc.aniso_state(), mc.aniso_result(), mc.result()
        assert (st["acnt"] == 4).all() and st["skipped"] == 0
        res.append({**st, **r, **{"vs." + k: v for k, v in vs.items()}})
        mc.free()
    for other in (1, 2):
        for k in res[0]:
            assert np.asarray(res[0][k]).tobytes() == np.asarray(res[other][k]).tobytes(), (other, k)


def test_recovery_with_the_real_forward(ctx):
    """1 000 + 1 000 steps, proposal 1, noise-free c with sigma_c 0.01, a1/a2 exact at the true Vs from a smooth Gc/Gs profile.
    x_ref = dazim_column_lsq at the true Vs.  Condition: |mean - x_ref| <= 3 std at no fewer than 95 % of the (cell, knot, Gc/Gs)
    entries, and the Vs uncertainty shows (std_between > 0 somewhere).
    Measured on an MI355X: the share is 1.000, the median std_between / std 0.036, sigma_a 1.65e-3, the run 12.6 s with 0.63 s in
    its 100 passes, no state skipped."""
    nx = ny = 8
    mc, truth, depz, periods, lsen, amap, Kin = disp_problem(ctx, nx, ny, 1, 1, 1)
    nlay, kmax = mc.nlay, mc.kmax
    # sigma_a a tenth of the RMS 2-psi term, and a weak regulariser: the solve at the true Vs fits a1/a2
    sigma_a = 0.1 * float(np.sqrt((amap.astype(np.float64) ** 2).mean()))
    wa = np.full((kmax, ny - 2, nx - 2), 1.0 / sigma_a, np.float32)
    nrm = np.sqrt((Kin ** 2).sum(axis=1)).max() / sigma_a
    smooth, damp = np.float32(0.1 * nrm), np.float32(0.0)
    x_ref, _, stats = ctx.column_lsq(nx, ny, nlay, lsen, amap, wa, smooth, damp)
    assert (stats[:, :, 1] <= 1.5 * sigma_a).all(), stats      # the misfit at the true Vs is of the size of sigma_a
    mc.set_aniso(10, amap, wa, smooth, damp)
    t0 = time.time()
    mc.run(depz, 3.0, periods, 1000, 1000)
    dt = time.time() - t0
    r = mc.aniso_result()
    assert (r["nsamp"] == 100 * mc.nchain).all() and ctx.stat("mc.aniso_passes") == 100
    inside = np.abs(r["mean"] - x_ref) <= 3 * r["std"]
    share = r["std_between"] / r["std"]
    print(f"\n[measured] |mean - x_ref| <= 3 std at {inside.mean():.3f} of the entries; median std_between / std {np.median(share):.3f}; "
          f"sigma_a {sigma_a:.2e}; run {dt:.2f} s (aniso passes {ctx.stat('mc.aniso'):.2f} s, skipped {ctx.stat('mc.aniso_skipped'):.0f})")
    assert inside.mean() >= 0.95
    assert (r["std_between"] > 0).any()
    mc.free()


def test_refusals(ctx):
    rng = np.random.default_rng(5)
    nlay, kmax, nchain = 3, 4, 8
    mc, cells, cobs, amap, wa = grid_problem(ctx, rng, nlay, kmax, nchain, 2)
    ncolc = mc.ncs * 4
    lsen = trend_kernels(rng, nlay, kmax, ncolc)

    def refused(fn, *a, **kw):
        with pytest.raises(dz.DazimError) as e:
            fn(*a, **kw)
        assert e.value.code == dz.DAZIM_E_BAD_ARG

    refused(mc.aniso_step, lsen)                                   # Gc/Gs not switched on
    refused(mc.aniso_result)
    refused(mc.set_aniso, -1, amap, wa, 1.0, 0.0)
    for v in (np.nan, np.inf):
        bad = amap.copy()
        bad[1, 2, 0, 1] = v
        refused(mc.set_aniso, 1, bad, wa, 1.0, 0.0)
        bad = wa.copy()
        bad[2, 1, 0] = v
        refused(mc.set_aniso, 1, amap, bad, 1.0, 0.0)
    refused(mc.set_aniso, 1, amap, wa, 0.0, 0.0)
    refused(mc.set_aniso, 1, amap, wa, -1.0, 1.0)
    refused(mc.set_aniso, 1, amap, wa, 1.0, -1.0)
    other = dz.Context(0)
    rc = other.lib.dazim_mc_set_aniso(other._h, mc._h, 1, dz._ptr(amap), dz._ptr(wa), 1.0, 0.0)
    assert rc == dz.DAZIM_E_BAD_ARG
    mc.set_aniso(3, amap, wa, 1.0, 0.0)
    mc.set_aniso(0)                                                # off again: the arrays are not looked at
    assert mc.aniso_state() == dict(nthin=0)
    refused(mc.aniso_step, lsen)
    mc.set_aniso(3, amap, wa, 1.0, 0.0)
    refused(mc.aniso_step, lsen)                                   # before the handle's first step
    mc.step(curves(rng, mc, cells, cobs, []), 0)
    refused(mc.set_aniso, 3, amap, wa, 1.0, 0.0)                   # once a step has been done
    refused(mc.set_aniso, 0)
    refused(mc.aniso_result)                                       # before the first sample
    refused(mc.aniso_step, lsen[:, :, :-1])                        # a wrong ncolc
    refused(mc.aniso_step, trend_kernels(rng, nlay, kmax + 1, ncolc))
    rc = other.lib.dazim_mc_aniso_step(other._h, mc._h, kmax, ncolc, dz._ptr(lsen))
    assert rc == dz.DAZIM_E_BAD_ARG
    rc = other.lib.dazim_mc_aniso_result(other._h, mc._h, None, None, None, None, None)
    assert rc == dz.DAZIM_E_BAD_ARG
    other.close()
    mc.aniso_step(lsen)                                            # the handle still works
    assert (mc.aniso_result()["nsamp"].reshape(-1)[cells] == 4).all()
    mc.free()
    # a handle without tempering set through mc_create's convenience
    mc2 = ctx.mc_create(5, 5, nlay + 1, kmax, 4, 8, 1, np.full((nlay + 1, 5, 5), 3.5, np.float32), np.full((nlay, 3, 3), 3.0, np.float32),
                        np.full((nlay, 3, 3), 4.0, np.float32), np.full((kmax, 3, 3), 3.5, np.float32), np.ones((kmax, 3, 3), np.float32),
                        aniso=dict(nthin=2, amap=amap, wa=wa, smooth=1.0, damp=0.0))
    assert mc2.aniso_state()["nthin"] == 2
    mc2.free()
