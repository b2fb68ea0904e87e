"""-m gpu: Monte-Carlo Vs per map cell (dazim_mc_*).

The step against its NumPy restatement (tests/mc_ref.py, driven by tests/mc_step_check.py) bit for bit, the sampler on a
linear-Gaussian problem with a known posterior and on the prior alone, reproducibility, recovery with the dispersion forward model,
cells without data and the refused arguments."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_ref
from tests.mc_step_check import check_final, drive

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    dz.build()
    c = dz.Context(0)
    yield c
    c.close()


def per_column(a, mc):
    """[n][ny-2][nx-2] per inner cell -> [n][ncol] per chain of the sampled cells (cells with data in cell order)"""
    a = a.reshape(a.shape[0], -1)
    return np.repeat(a[:, sampled_cells(mc)], mc.nchain, axis=1)


def sampled_cells(mc):
    return mc._cells


def create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, step=0.05, nadapt=50):
    mc = ctx.mc_create(nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, step, nadapt)
    mc._cells = np.nonzero((wdat.reshape(kmax, -1) != 0).any(axis=0))[0]
    assert len(mc._cells) == mc.ncs
    return mc


def test_one_step_against_numpy(ctx):
    """16 cells x 32 chains, 20 steps (10 burn-in with adaptation every 3, 10 recorded) on the same random curves on both sides, some
    of them 0 at weighted periods (the first step too: chains that start at chi^2 = +inf)"""
    rng = np.random.default_rng(11)
    nx = ny = 6
    nz, kmax, nchain, nbin, seed, nadapt = 6, 8, 32, 20, 0x1234_5678_9ABC, 3
    nlay, ncell = nz - 1, 16
    vel0 = rng.uniform(3.0, 4.5, (nz, ny, nx)).astype(np.float32)
    vmin = rng.uniform(2.8, 3.4, (nlay, ny - 2, nx - 2)).astype(np.float32)
    vmax = (vmin + rng.uniform(0.3, 1.2, vmin.shape)).astype(np.float32)
    cobs = rng.uniform(3.2, 4.0, (kmax, ny - 2, nx - 2)).astype(np.float32)
    wdat = np.where(rng.random((kmax, ny - 2, nx - 2)) < 0.2, 0.0, rng.uniform(50, 150, (kmax, ny - 2, nx - 2))).astype(np.float32)
    wdat[:, 0, 0] = 0.0
    wdat[3, 0, 0] = 80.0                        # a cell with one weighted period
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, 0.05, nadapt)
    assert mc.n_empty == 0 and mc.ncol == ncell * nchain
    lo, hi = per_column(vmin.astype(np.float64), mc), per_column(vmax.astype(np.float64), mc)
    cb, wd = per_column(cobs, mc), per_column(wdat, mc)
    gid = np.repeat(mc._cells, nchain) * nchain + np.tile(np.arange(nchain), ncell)
    prop = mc.proposals().cpu().numpy()
    assert np.array_equal(prop[:nlay], mc_ref.start_models(gid.astype(np.uint32), lo, hi, seed))
    assert np.array_equal(prop[nlay], per_column(vel0[nlay:, 1:-1, 1:-1], mc)[0])

    def forward(t):
        pv = (cb.astype(np.float64) + rng.normal(0, 0.012, cb.shape)).astype(np.float32).astype(np.float64)
        pv[rng.random(pv.shape) < (0.02 if t == 1 else 0.01)] = 0.0
        return pv

    run = drive(mc, forward, 10, 10, nadapt, lo, hi, cb, wd, nbin, seed, moved=True)
    got = run["got"]
    assert run["ninf0"] > 0 and run["ndec"] > 0  # both no-root rules and real decisions were exercised
    assert (got["scale"] != np.float32(0.05)).any()
    assert np.isfinite(got["best_chi2"]).all()
    # the posterior statistics of the 10 recorded steps against k_mc_final restated from the final state
    _, finite = check_final(mc, got, vmin, vmax, vel0, 1, 10, nbin)
    assert finite > 0.9
    mc.free()


def test_linear_gaussian_posterior(ctx):
    """c = K v (fp64, host): 64 cells, 4 knots, 32 chains, 2000 burn-in and 8000 recorded steps against the analytic posterior"""
    rng = np.random.default_rng(5)
    nx = ny = 10
    nz, kmax, nchain, nbin = 5, 6, 32, 64
    nlay, ncell = nz - 1, 64
    K = np.eye(kmax, nlay) + 0.35 * rng.random((kmax, nlay))
    sig = 0.02
    P = K.T @ K / sig ** 2
    cov = np.linalg.inv(P)
    assert np.linalg.cond(cov) <= 100
    sd = np.sqrt(np.diag(cov))
    vtrue = rng.uniform(3.0, 4.0, (ncell, nlay))
    cobs64 = vtrue @ K.T + rng.normal(0, sig, (ncell, kmax))
    cobs = cobs64.astype(np.float32)
    mu = (cobs.astype(np.float64) @ K / sig ** 2) @ cov           # [ncell][nlay]
    vmin = (mu - 6 * sd).astype(np.float32)
    vmax = (mu + 6 * sd).astype(np.float32)
    sh = (ny - 2, nx - 2)
    vel0 = np.full((nz, ny, nx), 3.5, np.float32)
    wdat = np.full((kmax,) + sh, 1.0 / sig, np.float32)
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, 77, vel0, vmin.T.reshape((nlay,) + sh), vmax.T.reshape((nlay,) + sh),
                cobs.T.reshape((kmax,) + sh), wdat)
    w32 = np.float64(np.float32(1.0 / sig))
    for t in range(10000):
        v = mc.proposals().cpu().numpy()[:nlay].astype(np.float64)
        mc.step(K @ v, int(t >= 2000))
    r = mc.result()
    # the posterior with the weights as the library holds them (fp32 1/sigma)
    P = K.T @ K * w32 ** 2
    cov = np.linalg.inv(P)
    sd = np.sqrt(np.diag(cov))
    mu = (cobs.astype(np.float64) @ K * w32 ** 2) @ cov
    mean = r["mean"].reshape(nlay, ncell).T
    std = r["std"].reshape(nlay, ncell).T
    dmean = np.abs(mean - mu) / sd
    dstd = np.abs(std / sd - 1)
    print(f"\n[measured] |mean - mu| / sigma max {dmean.max():.3f}; |std / sigma - 1| max {dstd.max():.3f}; "
          f"R-hat max {r['rhat'].max():.4f}; acceptance {r['accept'].min():.3f}..{r['accept'].max():.3f}")
    assert dmean.max() <= 0.1
    assert dstd.max() <= 0.1
    assert r["rhat"].max() < 1.05
    assert r["accept"].min() >= 0.15 and r["accept"].max() <= 0.45
    mc.free()


def prior_only(ctx, nx, ny, empty=()):
    rng = np.random.default_rng(3)
    nz, kmax, nchain, nbin = 4, 3, 32, 40
    nlay = nz - 1
    sh = (ny - 2, nx - 2)
    vel0 = rng.uniform(3.0, 4.0, (nz, ny, nx)).astype(np.float32)
    vmin = rng.uniform(2.5, 3.5, (nlay,) + sh).astype(np.float32)
    vmax = (vmin + rng.uniform(0.2, 1.5, vmin.shape)).astype(np.float32)
    wdat = np.full((kmax,) + sh, 1e-6, np.float32)
    for (j, i) in empty:
        wdat[:, j, i] = 0.0
    cobs = np.full((kmax,) + sh, 3.5, np.float32)
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, 9, vel0, vmin, vmax, cobs, wdat)
    return mc, vel0, vmin, vmax


def test_prior_only(ctx):
    """weights 1e-6: the posterior is the uniform box"""
    mc, vel0, vmin, vmax = prior_only(ctx, 6, 6)
    pv = np.full((mc.kmax, mc.ncol), 3.3, np.float64)
    for t in range(3300):
        mc.step(pv, int(t >= 300))
    r = mc.result()
    width = (vmax - vmin).astype(np.float64)
    mid = (vmin.astype(np.float64) + vmax) / 2
    print(f"\n[measured] |mean - mid| / width max {(np.abs(r['mean'] - mid) / width).max():.4f}; "
          f"|std / (width/sqrt 12) - 1| max {np.abs(r['std'] / (width / np.sqrt(12)) - 1).max():.4f}")
    assert (np.abs(r["mean"] - mid) <= 0.02 * width).all()
    assert (np.abs(r["std"] / (width / np.sqrt(12)) - 1) <= 0.05).all()
    for e, qv in enumerate((0.025, 0.5, 0.975)):
        assert (np.abs(r["q"][e] - (vmin + qv * width)) <= width / mc.nbin).all(), e
    mc.free()


def test_cells_without_data(ctx):
    """cells whose weights are all 0 are not sampled: their result is the start model exactly, std 0, and they are counted"""
    empty = [(0, 0), (2, 3), (3, 1)]
    mc, vel0, vmin, vmax = prior_only(ctx, 6, 7, empty)
    assert mc.n_empty == 3 and mc.ncol == (20 - 3) * mc.nchain
    pv = np.full((mc.kmax, mc.ncol), 3.3, np.float64)
    for t in range(20):
        mc.step(pv, int(t >= 10))
    r = mc.result()
    for (j, i) in empty:
        assert np.array_equal(r["mean"][:, j, i], vel0[:-1, j + 1, i + 1])
        assert (r["std"][:, j, i] == 0).all()
        assert np.array_equal(r["q"][:, :, j, i], np.broadcast_to(vel0[:-1, j + 1, i + 1], (3, mc.nlay)))
    other = np.ones(r["std"].shape[1:], bool)
    for (j, i) in empty:
        other[j, i] = False
    assert (r["std"][:, other] > 0).all()
    mc.free()


def disp_setup(ctx, nx, ny, sigma, seed=1):
    depz = np.array([0.0, 8.0, 20.0, 35.0, 60.0], np.float32)
    periods = np.array([6.0, 8.0, 10.0, 14.0, 18.0, 24.0, 30.0, 40.0])
    nz, kmax = len(depz), len(periods)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    truth = np.zeros((nz, ny, nx), np.float32)
    for k, z in enumerate(depz):
        truth[k] = 2.9 + 0.025 * z + 0.12 * np.sin(0.9 * ii + 0.5 * k) * np.cos(0.7 * jj)
    pv, _, nf = ctx.depthkernel(truth, depz, periods, 3.0, kernels=False)
    assert nf == 0
    cobs = pv.reshape(kmax, ny, nx)[:, 1:-1, 1:-1].astype(np.float32)
    mean = truth[:-1].mean(axis=(1, 2))
    vmin = np.broadcast_to((mean - 0.5)[:, None, None], (nz - 1, ny - 2, nx - 2)).astype(np.float32)
    vmax = np.broadcast_to((mean + 0.5)[:, None, None], (nz - 1, ny - 2, nx - 2)).astype(np.float32)
    wdat = np.full((kmax, ny - 2, nx - 2), 1.0 / sigma, np.float32)
    mc = create(ctx, nx, ny, nz, kmax, 16, 100, seed, truth, vmin, vmax, cobs, wdat)
    return mc, truth, depz, periods


def test_reproducible_runs(ctx):
    """two dazim_mc_run calls with one seed give the same bits; another seed gives other results"""
    res = []
    for seed in (4, 4, 5):
        mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, seed)
        mc.run(depz, 3.0, periods, 30, 40)
        res.append(mc.result())
        assert ctx.stat("mc.steps") == 70 and ctx.stat("mc") > 0 and ctx.stat("mc.disp") > 0
        mc.free()
    for k in res[0]:
        assert res[0][k].tobytes() == res[1][k].tobytes(), k
    assert not np.array_equal(res[0]["mean"], res[2]["mean"])


def test_dispersion_forward_recovery(ctx):
    """6 x 6 cells, 5 knots (4 sampled), 8 periods, exact curves of a laterally varying model: sigma_c 0.01 covers the truth; a
    four times smaller sigma_c halves the median posterior std at least"""
    out = {}
    for sigma in (0.01, 0.0025):
        mc, truth, depz, periods = disp_setup(ctx, 8, 8, sigma)
        nr = mc.run(depz, 3.0, periods, 2000, 2000)
        r = mc.result()
        t = truth[:-1, 1:-1, 1:-1]
        inside = ((r["q"][0] <= t) & (t <= r["q"][2])).mean()
        out[sigma] = (inside, float(np.median(r["std"])), r)
        print(f"\n[measured] sigma_c {sigma}: truth inside [p2.5, p97.5] for {inside:.3f} of (cell, knot); median std "
              f"{np.median(r['std']):.4f} km/s; R-hat median {np.median(r['rhat']):.3f}; acceptance {ctx.stat('mc.accept'):.3f}; "
              f"no root {nr}; run {ctx.stat('mc'):.2f} s (dispersion {ctx.stat('mc.disp'):.2f} s, steps {ctx.stat('mc.step'):.3f} s)")
        mc.free()
    assert out[0.01][0] >= 0.9
    assert out[0.0025][1] <= 0.5 * out[0.01][1]


def test_refused_arguments(ctx):
    nx = ny = 5
    nz, kmax = 4, 3
    sh = (ny - 2, nx - 2)
    vel0 = np.full((nz, ny, nx), 3.5, np.float32)
    vmin = np.full((nz - 1,) + sh, 3.0, np.float32)
    vmax = np.full((nz - 1,) + sh, 4.0, np.float32)
    cobs = np.full((kmax,) + sh, 3.5, np.float32)
    wdat = np.ones((kmax,) + sh, np.float32)
    good = dict(nx=nx, ny=ny, nz=nz, kmax=kmax, nchain=8, nbin=10, seed=1, vel0=vel0, vmin=vmin, vmax=vmax, cobs=cobs, wdat=wdat,
                step=0.05, nadapt=50)

    def refused(**kw):
        a = dict(good, **kw)
        with pytest.raises(dz.DazimError) as e:
            ctx.mc_create(**a)
        assert e.value.code == dz.DAZIM_E_BAD_ARG, kw.keys()

    refused(nchain=0)
    refused(nchain=65)
    refused(nz=1, vel0=vel0[:1], vmin=vmin[:0], vmax=vmax[:0])
    refused(nz=65, vel0=np.full((65, ny, nx), 3.5, np.float32), vmin=np.full((64,) + sh, 3.0, np.float32),
            vmax=np.full((64,) + sh, 4.0, np.float32))
    refused(kmax=0, cobs=cobs[:0], wdat=wdat[:0])
    refused(kmax=61, cobs=np.full((61,) + sh, 3.5, np.float32), wdat=np.ones((61,) + sh, np.float32))
    refused(nbin=1)
    bad = vmax.copy()
    bad[1, 2, 0] = 3.0
    refused(vmax=bad)
    refused(step=0.0)
    refused(step=-0.1)
    refused(step=0.6)                             # above the range the adaptation keeps
    refused(step=1e20)
    refused(step=float("inf"))
    refused(step=float("nan"))
    refused(nadapt=0)
    for name, arr in (("vmin", vmin), ("vmax", vmax), ("cobs", cobs), ("wdat", wdat)):
        for v in (-np.inf, np.inf, np.nan):
            bad = arr.copy()
            bad[0, 1, 2] = v
            refused(**{name: bad})
    ctx.mc_create(**dict(good, step=0.5)).free()  # the top of the range is accepted
    mc = ctx.mc_create(**good)
    for pv in (np.ones((kmax + 1, mc.ncol)), np.ones((kmax, mc.ncol - 1))):
        with pytest.raises(dz.DazimError) as e:
            mc.step(pv, 0)
        assert e.value.code == dz.DAZIM_E_BAD_ARG
    other = dz.Context(0)
    rc = other.lib.dazim_mc_step(other._h, mc._h, kmax, mc.ncol, dz._ptr(np.ones((kmax, mc.ncol))), 0)
    assert rc == dz.DAZIM_E_BAD_ARG
    other.close()
    mc.step(np.ones((kmax, mc.ncol)), 0)          # the handle still works
    mc.free()
