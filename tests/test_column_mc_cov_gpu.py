"""-m gpu: the covariance-adapted proposal of the Monte-Carlo sampler (dazim_mc_set_proposal kind 1).

The step against its NumPy restatement (tests/mc_ref.py, driven by tests/mc_step_check.py) at three shapes, the sampler on a
strongly correlated linear-Gaussian posterior against the isotropic proposal, the dispersion forward model in both kinds,
reproducibility, the unchanged default and the refused calls."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_ref
from tests.mc_step_check import drive
from tests.test_column_mc_gpu import create, disp_setup, per_column

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    dz.build()
    c = dz.Context(0)
    yield c
    c.close()


# (a): 11 knots = 66 pairs, more than one pass of the 64 lanes, and three Philox blocks; 3 x 32 = 96 >= 88 states, so the first
#      window factors.  (b): 3 chains x 4 steps = 12 states per window < 40: windows merge, the first factor comes at the fourth
#      adaptation point, from 3 chains' walks in 5 dimensions.  (max): the largest handle, 63 knots (2 016 pairs) and 64 chains, where the
#      step kernel's LDS is largest; 8 x 64 = 512 >= 504 states, so the first window factors.
@pytest.mark.parametrize("nz,nchain,nadapt,nburn,nrec", [(12, 32, 3, 12, 6), (6, 3, 4, 24, 4), (64, 64, 8, 18, 2)],
                         ids=["a", "b", "max"])
def test_one_step_against_numpy(ctx, nz, nchain, nadapt, nburn, nrec):
    """every step restated from the library's own state, proposals and cov_state, on random curves with some zeros at weighted periods"""
    rng = np.random.default_rng(11)
    nx = ny = 6
    kmax, nbin, seed = 8, 20, 0x1234_5678_9ABC
    nlay, ncell = nz - 1, 16
    vel0 = rng.uniform(3.0, 4.5, (nz, ny, nx)).astype(np.float32)
    vmin = rng.uniform(2.8, 3.4, (nlay, ny - 2, nx - 2)).astype(np.float32)
    vmax = (vmin + rng.uniform(0.3, 1.2, vmin.shape)).astype(np.float32)
    cobs = rng.uniform(3.2, 4.0, (kmax, ny - 2, nx - 2)).astype(np.float32)
    wdat = np.where(rng.random((kmax, ny - 2, nx - 2)) < 0.2, 0.0, rng.uniform(50, 150, (kmax, ny - 2, nx - 2))).astype(np.float32)
    wdat[:, 0, 0] = 0.0
    wdat[3, 0, 0] = 80.0
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, 0.05, nadapt)
    mc.set_proposal(1)
    assert mc.n_empty == 0 and mc.ncol == ncell * nchain
    lo, hi = per_column(vmin.astype(np.float64), mc), per_column(vmax.astype(np.float64), mc)
    cb, wd = per_column(cobs, mc), per_column(wdat, mc)
    cov0 = mc.cov_state()
    ref0 = mc_ref.empty_cov(ncell, nlay)
    for k in ref0:
        assert np.array_equal(cov0[k], ref0[k]), k
    root = np.sqrt(np.float32(nlay))

    def forward(t):
        pv = (cb.astype(np.float64) + rng.normal(0, 0.012, cb.shape)).astype(np.float32).astype(np.float64)
        pv[rng.random(pv.shape) < (0.02 if t == 1 else 0.01)] = 0.0
        return pv

    run = drive(mc, forward, nburn, nrec, nadapt, lo, hi, cb, wd, nbin, seed)
    got, gcov, nfact, first_factor_at = run["got"], run["gcov"], run["nfact"], run["first_factor_at"]
    print(f"\n[measured] nlay {nlay}, {nchain} chains: {nfact} factors, cond(C) max {max(run['conds']):.3g}; first factor after "
          f"{first_factor_at} burn-in decisions; scale {got['scale'].min():.4f}..{got['scale'].max():.4f}")
    assert run["before"] > 0 and run["after"] > 0            # decisions from isotropic and from covariance proposals
    assert (gcov["cov_set"] == 1).all() and nfact >= ncell
    assert first_factor_at == (nadapt if nchain * nadapt >= 8 * nlay else nadapt * -(-8 * nlay // (nchain * nadapt)))
    assert (got["scale"] <= np.float32(2.0) / root).all()
    mc.free()


def linear_problem():
    """16 cells, 8 knots, 10 periods: c = K v with a common column in K, so that the knots trade off against each other"""
    rng = np.random.default_rng(5)
    nx = ny = 6
    nz, kmax, nchain, nbin = 9, 10, 32, 64
    nlay, ncell = nz - 1, 16
    K = np.eye(kmax, nlay) + 0.35 * rng.random((kmax, nlay)) + 3.0 * np.ones((kmax, 1)) * rng.random((1, nlay))
    sig = 0.02
    w32 = np.float64(np.float32(1.0 / sig))
    cov = np.linalg.inv(K.T @ K * w32 ** 2)
    sd = np.sqrt(np.diag(cov))
    corr = cov / np.outer(sd, sd)
    assert np.linalg.cond(corr) >= 300, np.linalg.cond(corr)
    vtrue = rng.uniform(3.0, 4.0, (ncell, nlay))
    cobs = (vtrue @ K.T + rng.normal(0, sig, (ncell, kmax))).astype(np.float32)
    mu = (cobs.astype(np.float64) @ K * w32 ** 2) @ cov
    return dict(nx=nx, ny=ny, nz=nz, kmax=kmax, nchain=nchain, nbin=nbin, nlay=nlay, ncell=ncell, K=K, sig=sig, sd=sd, mu=mu, cobs=cobs,
                cond=np.linalg.cond(corr))


def test_correlated_linear_gaussian_posterior(ctx):
    """1500 burn-in and 3000 recorded steps against the analytic posterior in both kinds, one seed: kind 1 meets the bars of
    test_linear_gaussian_posterior and mixes better than kind 0"""
    p = linear_problem()
    nlay, ncell, kmax, K = p["nlay"], p["ncell"], p["kmax"], p["K"]
    sh = (p["ny"] - 2, p["nx"] - 2)
    vmin = (p["mu"] - 6 * p["sd"]).astype(np.float32)
    vmax = (p["mu"] + 6 * p["sd"]).astype(np.float32)
    vel0 = np.full((p["nz"], p["ny"], p["nx"]), 3.5, np.float32)
    wdat = np.full((kmax,) + sh, 1.0 / p["sig"], np.float32)
    out = {}
    for kind in (0, 1):
        mc = ctx.mc_create(p["nx"], p["ny"], p["nz"], kmax, p["nchain"], p["nbin"], 77, vel0, vmin.T.reshape((nlay,) + sh),
                           vmax.T.reshape((nlay,) + sh), p["cobs"].T.reshape((kmax,) + sh), wdat, proposal=kind)
        for t in range(4500):
            v = mc.proposals().cpu().numpy()[:nlay].astype(np.float64)
            mc.step(K @ v, int(t >= 1500))
        r = mc.result()
        scale = mc.state()["scale"]
        nset = int(mc.cov_state()["cov_set"].sum()) if kind else 0
        dmean = np.abs(r["mean"].reshape(nlay, ncell).T - p["mu"]) / p["sd"]
        dstd = np.abs(r["std"].reshape(nlay, ncell).T / p["sd"] - 1)
        out[kind] = (dmean.max(), dstd.max(), float(r["rhat"].max()), r["accept"].min(), r["accept"].max())
        print(f"\n[measured] kind {kind} (cond of the posterior correlation {p['cond']:.0f}): |mean - mu| / sigma max {dmean.max():.3f}; "
              f"|std / sigma - 1| max {dstd.max():.3f}; R-hat max {r['rhat'].max():.4f}; acceptance {r['accept'].min():.3f}.."
              f"{r['accept'].max():.3f}; scale {scale.min():.4f}..{scale.max():.4f}; cells with a factor {nset}")
        mc.free()
    dmean, dstd, rhat, amin, amax = out[1]
    assert dmean <= 0.1
    assert dstd <= 0.1
    assert rhat < 1.05
    assert amin >= 0.15 and amax <= 0.45
    assert rhat < out[0][2]


def test_dispersion_forward_both_kinds(ctx):
    """disp_setup's problem, 1000 + 1000 steps: kind 1 covers the truth as kind 0 must in test_dispersion_forward_recovery"""
    inside = {}
    for kind in (0, 1):
        mc, truth, depz, periods = disp_setup(ctx, 8, 8, 0.01)
        mc.set_proposal(kind)
        nr = mc.run(depz, 3.0, periods, 1000, 1000)
        r = mc.result()
        t = truth[:-1, 1:-1, 1:-1]
        inside[kind] = ((r["q"][0] <= t) & (t <= r["q"][2])).mean()
        assert ctx.stat("mc.proposal") == kind
        print(f"\n[measured] kind {kind}: truth inside [p2.5, p97.5] for {inside[kind]:.3f} of (cell, knot); R-hat median "
              f"{np.median(r['rhat']):.3f}, max {r['rhat'].max():.3f}; acceptance {ctx.stat('mc.accept'):.3f}; cells with a factor "
              f"{ctx.stat('mc.cov_cells'):.0f} of {mc.ncs}; no root {nr}; run {ctx.stat('mc'):.2f} s (dispersion "
              f"{ctx.stat('mc.disp'):.2f} s, steps {ctx.stat('mc.step'):.3f} s)")
        assert ctx.stat("mc.cov_cells") == (mc.ncs if kind else 0)
        mc.free()
    assert inside[1] >= 0.9


def test_reproducible_and_default_unchanged(ctx):
    """two kind-1 runs with one seed give the same bytes (120 + 40 steps: two adaptation points, both with a factor); after 30 + 40
    steps set_proposal(0) is the untouched handle"""
    res = {}
    for name, kind, nburn in (("a", 1, 120), ("b", 1, 120), ("zero", 0, 30), ("plain", None, 30), ("plain120", None, 120)):
        mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, 4)
        if kind is not None:
            mc.set_proposal(kind)
        mc.run(depz, 3.0, periods, nburn, 40)
        res[name] = {"result." + k: v for k, v in mc.result().items()}
        res[name].update({"state." + k: v for k, v in mc.state().items() if k != "step"})
        if kind == 1:
            res[name].update({"cov." + k: v for k, v in mc.cov_state().items() if k != "kind"})
        mc.free()
    for k in res["a"]:
        assert res["a"][k].tobytes() == res["b"][k].tobytes(), k
    for k in res["plain"]:
        assert res["zero"][k].tobytes() == res["plain"][k].tobytes(), k
    assert (res["a"]["cov.cov_set"] == 1).all()
    assert not np.array_equal(res["a"]["result.mean"], res["plain120"]["result.mean"])


def test_refusals(ctx):
    nx = ny = 5
    nz, kmax = 4, 3
    sh = (ny - 2, nx - 2)
    args = dict(nx=nx, ny=ny, nz=nz, kmax=kmax, nchain=8, nbin=10, seed=1, vel0=np.full((nz, ny, nx), 3.5, np.float32),
                vmin=np.full((nz - 1,) + sh, 3.0, np.float32), vmax=np.full((nz - 1,) + sh, 4.0, np.float32),
                cobs=np.full((kmax,) + sh, 3.5, np.float32), wdat=np.ones((kmax,) + sh, np.float32), step=0.05, nadapt=50)
    mc = ctx.mc_create(**args)
    pv = np.full((kmax, mc.ncol), 3.4)

    def refused(call):
        with pytest.raises(dz.DazimError) as e:
            call()
        assert e.value.code == dz.DAZIM_E_BAD_ARG

    refused(lambda: mc.set_proposal(2))
    refused(lambda: mc.set_proposal(-1))
    assert mc.cov_state() == dict(kind=0)
    s2 = np.zeros((mc.ncs, 6))
    rc = ctx.lib.dazim_mc_cov_state(ctx._h, mc._h, None, None, None, dz._ptr(s2), None, None)   # an array of a kind-0 handle
    assert rc == dz.DAZIM_E_BAD_ARG
    other = dz.Context(0)
    assert other.lib.dazim_mc_set_proposal(other._h, mc._h, 1) == dz.DAZIM_E_BAD_ARG
    assert other.lib.dazim_mc_cov_state(other._h, mc._h, None, None, None, None, None, None) == dz.DAZIM_E_BAD_ARG
    other.close()
    mc.set_proposal(1)                            # the handle still works: kind 1, back to 0, to 1 again, then steps
    mc.set_proposal(0)
    mc.set_proposal(1)
    assert mc.cov_state()["kind"] == 1
    mc.step(pv, 0)
    refused(lambda: mc.set_proposal(0))           # after a step
    refused(lambda: mc.set_proposal(1))
    mc.step(pv, 0)
    cov = mc.cov_state()
    assert cov["kind"] == 1 and (cov["cov_n"] == 8).all()
    mc.free()
