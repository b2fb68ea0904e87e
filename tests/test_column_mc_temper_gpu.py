"""-m gpu: parallel tempering of the Monte-Carlo sampler (dazim_mc_set_tempering).

The tempered step against its NumPy restatement (tests/mc_ref.py, driven by tests/mc_step_check.py) in both proposal kinds at five
shapes, a bimodal posterior that the untempered chains cannot cross, the unchanged default and reproducibility, the dispersion
forward model, and the refused calls."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_ref
from tests.mc_step_check import check_final, drive
from tests.test_column_mc_gpu import create, disp_setup, per_column

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    dz.build()
    c = dz.Context(0)
    yield c
    c.close()


NADAPT, NREC = 3, 4
# nburn for (kind 0, kind 1): kind 0 crosses two adaptation points; kind 1 goes on to the adaptation point at which the rung-0 chains
# (ncold per burn-in decision) have given the 8 nlay states of the first factor, and one window beyond it
SHAPES = {  # (nz, nchain, ntemp, nswap): nburn
    "plain": ((12, 32, 4, 1), (8, 16)),        # 88 states / 8 cold chains = 11 decisions: the factor at the 12th
    "odd": ((6, 6, 3, 2), (8, 25)),            # 40 / 2 = 20 decisions: the 21st
    "full": ((64, 64, 8, 1), (8, 67)),         # 504 / 8 = 63 decisions: the 63rd
    "one_group": ((3, 8, 8, 1), (8, 22)),      # 16 / 1 = 16 decisions: the 18th
    "groups32": ((5, 64, 2, 3), (8, 8)),       # 32 / 32 = 1 decision: the 3rd
}


def step_problem(nz):
    """the random cells of test_column_mc_gpu.test_one_step_against_numpy with one cell without data"""
    rng = np.random.default_rng(11)
    nx = ny = 6
    kmax = 8
    nlay = nz - 1
    vel0 = rng.uniform(3.0, 4.5, (nz, ny, nx)).astype(np.float32)
    vmin = rng.uniform(2.8, 3.4, (nlay, ny - 2, nx - 2)).astype(np.float32)
    vmax = (vmin + rng.uniform(0.3, 1.2, vmin.shape)).astype(np.float32)
    cobs = rng.uniform(3.2, 4.0, (kmax, ny - 2, nx - 2)).astype(np.float32)
    wdat = np.where(rng.random((kmax, ny - 2, nx - 2)) < 0.2, 0.0, rng.uniform(50, 150, (kmax, ny - 2, nx - 2))).astype(np.float32)
    wdat[:, 0, 0] = 0.0
    wdat[3, 0, 0] = 80.0
    wdat[:, 1, 2] = 0.0                         # a cell without data
    return rng, nx, ny, kmax, vel0, vmin, vmax, cobs, wdat


def host_forward(rng, cb, t, nswap):
    """the curves of step t: the observations plus noise, and no root (c = 0) at one period of 75 % of the columns up to the second
    swap round (5 % later), so that chains stay at chi^2 = +inf long enough to meet every case of the swap rule"""
    pv = (cb.astype(np.float64) + rng.normal(0, 0.012, cb.shape)).astype(np.float32).astype(np.float64)
    cols = np.nonzero(rng.random(cb.shape[1]) < (0.75 if t <= 2 * nswap else 0.05))[0]
    pv[rng.integers(0, cb.shape[0], cols.size), cols] = 0.0
    return pv


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tempered_step_against_numpy(ctx, shape, kind):
    """every step restated from the library's own state, ladder, proposals and cov_state: the fields and the allowances of
    test_one_step_against_numpy in both kinds, the scale of every rung and the swap counters"""
    (nz, nchain, ntemp, nswap), nburns = SHAPES[shape]
    nburn = nburns[kind]
    rng, nx, ny, kmax, vel0, vmin, vmax, cobs, wdat = step_problem(nz)
    nbin, seed, tmax = 20, 0x1234_5678_9ABC, 16.0
    nlay, ncs, ncold = nz - 1, 15, nchain // ntemp
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, 0.05, NADAPT)
    if kind == 1:                               # the two setters in either order
        mc.set_proposal(1)
    mc.set_tempering(ntemp, tmax, nswap)
    if kind == 0 and shape == "odd":
        mc.set_proposal(1)
        mc.set_proposal(0)
    assert mc.n_empty == 1 and mc.ncs == ncs and mc.ncol == ncs * nchain
    tp = mc.temper_state()
    assert (tp["ntemp"], tp["tmax"], tp["nswap"]) == (ntemp, tmax, nswap)
    assert np.abs(tp["beta"] / mc_ref.ladder(ntemp, tmax) - 1).max() <= 1e-14 and tp["beta"][0] == 1.0
    assert (tp["scale"] == np.float32(0.05)).all() and not tp["swap_try"].any() and not tp["swap_acc"].any()
    lo, hi = per_column(vmin.astype(np.float64), mc), per_column(vmax.astype(np.float64), mc)
    cb, wd = per_column(cobs, mc), per_column(wdat, mc)
    run = drive(mc, lambda t: host_forward(rng, cb, t, nswap), nburn, NREC, NADAPT, lo, hi, cb, wd, nbin, seed)
    got, gtp, gcov, seen, nfact = run["got"], run["gtp"], run["gcov"], run["seen"], run["nfact"]
    nswapped = int(gtp["swap_acc"].sum())
    hot = (np.arange(mc.ncol) % nchain) % ntemp != 0
    assert not got["sums"][:, :, hot].any() and not got["accepted"][hot].any()       # the columns of the hot chains stay 0
    assert got["hist"].sum() == NREC * nlay * ncs * ncold
    rounds = sum(1 for t in range(2, nburn + NREC + 1) if t % nswap == 0)
    assert gtp["swap_try"].sum() >= rounds * ncs * (nchain // ntemp) * ((ntemp - 1) // 2)
    assert all(seen[k] > 0 for k in seen), seen                  # every case of the swap rule, in the restatement's own run
    assert 0 < nswapped < gtp["swap_try"].sum()
    assert len(np.unique(gtp["scale"])) > 1                      # the rungs' scales went their own ways
    if kind == 1:
        assert (gcov["cov_set"] == 1).all() and nfact >= ncs
    print(f"\n[measured] {shape}, kind {kind}: swap cases {seen}; swaps {nswapped} of {gtp['swap_try'].sum()}; scale "
          f"{gtp['scale'].min():.4f}..{gtp['scale'].max():.4f}; {nfact} factors, cond(C) max {max(run['conds'] + [1.0]):.3g}")
    # the posterior statistics of the recorded steps against k_mc_final restated over the rung-0 chains
    r, _ = check_final(mc, got, vmin, vmax, vel0, ntemp, NREC, nbin)
    if ncold == 1:
        assert np.isnan(r["rhat"]).all()
    mc.free()


def bimodal_mass(w32):
    """the posterior mass below 3.5 of chi2 = (w (0.25 - c(v)))^2 on [2.5, 4.5], c = x^2 left of x = v - 3.5 = 0 and 4 x^2 right of
    it, by the midpoint rule on 2^20 cells per side (the integrand is smooth on each side)"""
    n = 1 << 20
    xl = -1.0 + (np.arange(n) + 0.5) / n
    xr = (np.arange(n) + 0.5) / n
    left = np.exp(-0.5 * (w32 * (0.25 - xl * xl)) ** 2).sum() / n
    right = np.exp(-0.5 * (w32 * (0.25 - 4.0 * xr * xr)) ** 2).sum() / n
    return left / (left + right)


def test_bimodal_target(ctx):
    """one knot, modes at 3.0 and 3.75 behind a barrier of chi^2 = 39, left-mode mass 2/3: 1000 + 3000 steps with 4 rungs up to
    T = 16 put every cell's mass below 3.5 within 0.06 of the quadrature; the same problem and seed without tempering does not"""
    nx = ny = 6
    nz, kmax, nchain, nbin, seed = 2, 1, 32, 64, 2024
    sh = (ny - 2, nx - 2)
    vel0 = np.full((nz, ny, nx), 3.5, np.float32)
    vmin, vmax = np.full((1,) + sh, 2.5, np.float32), np.full((1,) + sh, 4.5, np.float32)
    cobs, wdat = np.full((kmax,) + sh, 0.25, np.float32), np.full((kmax,) + sh, 1.0 / 0.04, np.float32)
    w32 = np.float64(np.float32(1.0 / 0.04))
    assert abs((w32 * 0.25) ** 2 - 39.0) < 0.1               # the barrier at x = 0
    mass = bimodal_mass(w32)
    assert abs(mass - 2.0 / 3.0) < 0.01, mass
    out = {}
    for ntemp in (4, 1):
        mc = ctx.mc_create(nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, ntemp=ntemp, tmax=16.0, nswap=1)
        for t in range(4000):
            x = mc.proposals().cpu().numpy()[:1].astype(np.float64) - 3.5
            mc.step(np.where(x < 0, x * x, 4.0 * x * x), int(t >= 1000))
        h = mc.state()["hist"][:, 0, :].astype(np.float64)        # bins of width 2 / 64: 3.5 is the edge between bins 31 and 32
        left = h[:, :32].sum(axis=1) / h.sum(axis=1)
        rhat = mc.result()["rhat"].ravel()
        out[ntemp] = (left, rhat)
        if ntemp > 1:
            tp = mc.temper_state()
            swap = tp["swap_acc"] / tp["swap_try"]
            assert (h.sum(axis=1) == 3000 * (nchain // ntemp)).all()
        mc.free()
        print(f"\n[measured] ntemp {ntemp}: left-mode mass {left.min():.3f}..{left.max():.3f} (quadrature {mass:.4f}); R-hat median "
              f"{np.median(rhat):.3f}, max {rhat.max():.3f}"
              + (f"; swap acceptance {swap.min():.3f}..{swap.max():.3f}" if ntemp > 1 else ""))
    left, rhat = out[4]
    assert np.abs(left - mass).max() <= 0.06
    assert rhat.max() <= 1.05
    assert swap.min() >= 0.3 and swap.max() <= 0.95
    left, rhat = out[1]                                      # the control: without tempering the problem is hard
    assert np.abs(left - mass).max() > 0.15
    assert np.median(rhat) > 5


def everything(mc):
    out = {"result." + k: v for k, v in mc.result().items()}
    out.update({"state." + k: v for k, v in mc.state().items() if k != "step"})
    out.update({"cov." + k: v for k, v in mc.cov_state().items() if k != "kind"})
    out.update({"temper." + k: v for k, v in mc.temper_state().items() if isinstance(v, np.ndarray)})
    return out


def test_default_unchanged_and_reproducible(ctx):
    """set_tempering(1, ..) is the untouched handle bit for bit in both kinds (120 + 40 steps: kind 1 factors); two tempered runs
    with one seed give the same bytes; a cell's tempered result does not depend on which other cells have data"""
    res = {}
    for name, kind, ntemp in (("plain0", 0, None), ("one0", 0, 1), ("plain1", 1, None), ("one1", 1, 1), ("a", 1, 4), ("b", 1, 4)):
        mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, 4)
        mc.set_proposal(kind)
        if ntemp == 1:
            mc.set_tempering(4, 16.0, 2)                      # and back to the default
            mc.set_tempering(1, 1.0, 1)
            assert mc.temper_state() == dict(ntemp=1, tmax=1.0, nswap=1)
        elif ntemp:
            mc.set_tempering(ntemp, 16.0, 1)
        mc.run(depz, 3.0, periods, 120, 40)
        assert ctx.stat("mc.ntemp") == (ntemp or 1)
        res[name] = everything(mc)
        mc.free()
    for kind in "01":
        assert res["plain" + kind].keys() == res["one" + kind].keys()
        for k in res["plain" + kind]:
            assert res["plain" + kind][k].tobytes() == res["one" + kind][k].tobytes(), (kind, k)
    assert res["a"].keys() == res["b"].keys() and "temper.swap_acc" in res["a"] and "cov.chol" in res["a"]
    for k in res["a"]:
        assert res["a"][k].tobytes() == res["b"][k].tobytes(), k
    assert res["a"]["temper.swap_acc"].sum() > 0
    assert not np.array_equal(res["a"]["result.mean"], res["plain1"]["result.mean"])
    # the cells: 16 of them, then the same with three cells' weights at 0; host curves that depend on the column's own model only
    rng = np.random.default_rng(8)
    nx = ny = 6
    nz, kmax, nchain, nbin = 4, 3, 16, 20
    sh = (ny - 2, nx - 2)
    vel0 = np.full((nz, ny, nx), 3.5, np.float32)
    vmin = rng.uniform(2.8, 3.2, (nz - 1,) + sh).astype(np.float32)
    vmax = (vmin + rng.uniform(0.5, 1.0, vmin.shape)).astype(np.float32)
    cobs = rng.uniform(3.3, 3.6, (kmax,) + sh).astype(np.float32)
    K = rng.uniform(0.2, 0.5, (kmax, nz - 1))
    r = {}
    for name, empty in (("all", ()), ("some", ((0, 1), (2, 2), (3, 0)))):
        wdat = np.full((kmax,) + sh, 40.0, np.float32)
        for (j, i) in empty:
            wdat[:, j, i] = 0.0
        mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, 21, vel0, vmin, vmax, cobs, wdat, 0.05, 10)
        mc.set_tempering(4, 8.0, 1)
        for t in range(60):
            v = mc.proposals().cpu().numpy()[:nz - 1].astype(np.float64)
            mc.step(K @ v, int(t >= 40))
        r[name] = (mc.result(), mc._cells, mc.temper_state())
        mc.free()
    keep = np.ones(sh, bool)
    for (j, i) in ((0, 1), (2, 2), (3, 0)):
        keep[j, i] = False
    for k in r["all"][0]:
        assert r["all"][0][k][..., keep].tobytes() == r["some"][0][k][..., keep].tobytes(), k
    rows = np.isin(r["all"][1], r["some"][1])
    for k in ("scale", "swap_try", "swap_acc"):
        assert np.array_equal(r["all"][2][k][rows], r["some"][2][k]), k


def test_dispersion_forward_tempered(ctx):
    """disp_setup's 6 x 6 cells through dazim_mc_run, 16 chains in 4 rungs, kind 1, 300 + 300 steps: the truth inside the interval of
    the 4 recorded chains of every cell"""
    mc, truth, depz, periods = disp_setup(ctx, 8, 8, 0.01)
    mc.set_proposal(1)
    mc.set_tempering(4, 16.0, 1)
    nr = mc.run(depz, 3.0, periods, 300, 300)
    r = mc.result()
    tp = mc.temper_state()
    t = truth[:-1, 1:-1, 1:-1]
    inside = (r["q"][0] <= t) & (t <= r["q"][2])
    swap = tp["swap_acc"] / tp["swap_try"]
    print(f"\n[measured] ntemp 4, kind 1: truth inside [p2.5, p97.5] for {inside.mean():.3f} of (cell, knot); R-hat median "
          f"{np.median(r['rhat']):.3f}, max {r['rhat'].max():.3f}; acceptance {ctx.stat('mc.accept'):.3f}; swap acceptance min "
          f"{ctx.stat('mc.swap_min'):.3f}, median {ctx.stat('mc.swap_med'):.3f}; no root {nr}; run {ctx.stat('mc'):.2f} s (dispersion "
          f"{ctx.stat('mc.disp'):.2f} s, steps {ctx.stat('mc.step'):.3f} s)")
    assert inside.all(axis=0).all()
    assert ctx.stat("mc.ntemp") == 4
    assert ctx.stat("mc.swap_min") > 0
    assert ctx.stat("mc.swap_min") == swap.min() and ctx.stat("mc.swap_med") == np.median(swap)
    assert abs(ctx.stat("mc.accept") - r["accept"].mean()) < 1e-6
    mc.free()


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

    for ntemp in (3, 5, 16, 0, -2):                            # no divisor of 8 chains, above them, below 1
        refused(lambda: mc.set_tempering(ntemp, 16.0, 1))
    for tmax in (1.0, 0.5, 0.0, -4.0, float("inf"), float("nan")):
        refused(lambda: mc.set_tempering(4, tmax, 1))
    for nswap in (0, -1):
        refused(lambda: mc.set_tempering(4, 16.0, nswap))
        refused(lambda: mc.set_tempering(1, 16.0, nswap))
    refused(lambda: ctx.mc_create(**args, ntemp=3, tmax=16.0))
    assert mc.temper_state() == dict(ntemp=1, tmax=1.0, nswap=1)
    for i in range(4):                                         # an array of an untempered handle
        arrs = [None] * 4
        arrs[i] = dz._ptr(np.zeros(mc.ncs * 8))
        assert ctx.lib.dazim_mc_temper_state(ctx._h, mc._h, None, None, None, *arrs) == dz.DAZIM_E_BAD_ARG
    other = dz.Context(0)
    assert other.lib.dazim_mc_set_tempering(other._h, mc._h, 4, 16.0, 1) == dz.DAZIM_E_BAD_ARG
    assert other.lib.dazim_mc_temper_state(other._h, mc._h, None, None, None, None, None, None, None) == dz.DAZIM_E_BAD_ARG
    other.close()
    mc.set_tempering(1, 0.5, 1)                                # ntemp 1 does not look at tmax
    mc.set_tempering(4, 16.0, 2)                               # the handle still works: a ladder, another, then steps
    mc.set_tempering(2, 4.0, 1)
    tp = mc.temper_state()
    assert (tp["ntemp"], tp["tmax"], tp["nswap"]) == (2, 4.0, 1) and np.array_equal(tp["beta"], [1.0, 0.25])
    assert tp["scale"].shape == (mc.ncs, 2) and tp["swap_try"].shape == (mc.ncs, 1)
    mc.step(pv, 0)
    refused(lambda: mc.set_tempering(2, 4.0, 1))               # after a step
    refused(lambda: mc.set_tempering(1, 1.0, 1))
    mc.step(pv, 0)
    tp = mc.temper_state()
    assert (tp["swap_try"] == 4).all()                         # step 2, round 2: the pair (0, 1) of each of the 4 groups
    mc.free()
