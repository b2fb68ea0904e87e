"""-m gpu: the Gaussian smoothness prior of the Monte-Carlo sampler (dazim_mc_set_prior).

The step with E + Q against its NumPy restatement (tests/mc_ref.py with tests/mc_prior_ref.py's Q, driven by tests/mc_step_check.py) in all eight mode
triples; a linear-Gaussian problem that the data alone do not determine, on which the chains, dazim_column_lsq and
dazim_column_resolution stand against one analytic posterior; the unchanged default; the dispersion forward model with and without
the prior; and the refused calls."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_prior_ref
from tests.bars import within
from tests.mc_step_check import check_final, drive
from tests.test_column_mc_gpu import create, disp_setup, per_column
from tests.test_column_mc_noise_gpu import everything
from tests.test_column_mc_temper_gpu import host_forward, step_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    dz.build()
    c = dz.Context(0)
    yield c
    c.close()


NADAPT, NBURN, NREC = 3, 10, 10
SMOOTH, DAMP = 3.0, 4.0
# (nz, nchain, ntemp, nswap, kind, noise); between them every (kind, tempered, noise) triple.  Kind 1 reaches its first factor inside
# the 9 burn-in decisions: 8 nlay states over the rung-0 chains are 6 decisions at "two", 8 at "four", 5 at "nine", 4 at "two5"
SHAPES = {
    "one": (2, 1, 1, 1, 0, 0),            # nlay 1, one chain
    "two": (3, 3, 1, 1, 1, 0),            # nlay 2, 3 chains
    "three": (4, 6, 3, 1, 0, 0),          # nlay 3, 6 chains, 3 rungs, a swap round every step: both parities
    "five": (6, 32, 1, 1, 0, 1),          # nlay 5, 32 chains
    "nine": (10, 64, 4, 1, 1, 1),         # nlay 9, 64 chains, 4 rungs, kind 1, noise on
    "four": (5, 8, 2, 1, 1, 0),
    "three2": (4, 6, 2, 2, 0, 1),
    "two5": (3, 5, 1, 1, 1, 1),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_prior_step_against_numpy(ctx, shape):
    """10 burn-in steps (adaptation every 3) and 10 recorded ones on hand-made curves, every step restated from the library's own
    state: what tests/mc_step_check.drive compares, and prior_state()'s q bit for bit against the restated step's and against Q of
    the new states.  smooth 3, damp 4 about a random reference inside the boxes put the differences of Q beside those of chi2: some
    decisions, and with a ladder some swaps, come out otherwise than chi2 alone would have made them."""
    nz, nchain, ntemp, nswap, kind, noise = SHAPES[shape]
    rng, nx, ny, kmax, vel0, vmin, vmax, cobs, wdat = step_problem(nz)
    nbin, seed, tmax = 20, 0x1234_5678_9ABC, 16.0
    nlay = nz - 1
    vref = (vmin + np.random.default_rng(nz).uniform(0.1, 0.9, vmin.shape) * (vmax - vmin)).astype(np.float32)
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, 0.05, NADAPT)
    if shape in ("one", "nine"):                # the setters in either order
        mc.set_prior(SMOOTH, DAMP, vref)
    if kind == 1:
        mc.set_proposal(1)
    if ntemp > 1:
        mc.set_tempering(ntemp, tmax, nswap)
    if noise:
        mc.set_noise(0.25, 0.5)
    if shape not in ("one", "nine"):
        mc.set_prior(1.0, 0.0)                  # a second call replaces the prior
        mc.set_prior(SMOOTH, DAMP, vref)
    ps = mc.prior_state()
    assert (ps["smooth"], ps["damp"]) == (SMOOTH, DAMP) and np.array_equal(ps["vref"], vref) and ps["q"].shape == (mc.ncol,)
    lo, hi = per_column(vmin.astype(np.float64), mc), per_column(vmax.astype(np.float64), mc)
    cb, wd, vr = per_column(cobs, mc), per_column(wdat, mc), per_column(vref, mc)
    # before the first step the states are the start models
    assert np.array_equal(ps["q"], mc_prior_ref.prior_q(mc.state()["cur"][:nlay], vr, SMOOTH, DAMP))
    run = drive(mc, lambda t: host_forward(rng, cb, t, nswap), NBURN, NREC, NADAPT, lo, hi, cb, wd, nbin, seed, vref=vr)
    got, gtp, gcov, gpr, seen = run["got"], run["gtp"], run["gcov"], run["gpr"], run["seen"]
    q = gpr["q"]
    print(f"\n[measured] {shape}: decisions {run['ndec']} accepted, {run['ndiff_dec']} other than chi2 alone; swaps "
          f"{int(gtp['swap_acc'].sum())} of {int(gtp['swap_try'].sum())}, {run['ndiff_swap']} rules other than chi2 alone; Q "
          f"{q.min():.2f}..{q.max():.2f} beside chi2 {got['chi2'][np.isfinite(got['chi2'])].min():.2f}.."
          f"{np.median(got['chi2'][np.isfinite(got['chi2'])]):.2f} (median); swap cases {seen}")
    assert run["ndec"] > 0 and run["ndiff_dec"] > 0
    if ntemp > 1:
        assert run["ndiff_swap"] > 0 and 0 < gtp["swap_acc"].sum() < gtp["swap_try"].sum()
        assert seen["both_finite"] > 0 and seen["lower_inf"] + seen["upper_inf"] + seen["both_inf"] > 0
    if kind == 1:
        assert (gcov["cov_set"] == 1).all() and run["nfact"] >= mc.ncs
    if noise:
        assert run["gns"]["ncnt"].sum() > 0
    # the Vs statistics are those of the recorded states, as without the prior
    check_final(mc, got, vmin, vmax, vel0, ntemp, NREC, nbin, roots=False)
    mc.free()


def linear_problem():
    """test_linear_gaussian_posterior's construction with 3 periods for 5 knots: c = K v, sigma 0.02, and the prior smooth 5,
    damp 5 about 3.5.  The posterior is the Gaussian of precision A = K^T W^2 K + P with mean vref + A^-1 K^T W^2 (cobs - K vref)"""
    rng = np.random.default_rng(5)
    ncell, kmax, nlay, sig, smooth, damp = 64, 3, 5, 0.02, 5.0, 5.0
    K = np.eye(kmax, nlay) + 0.35 * rng.random((kmax, nlay))
    vtrue = rng.uniform(3.0, 4.0, (ncell, nlay))
    cobs = (vtrue @ K.T + rng.normal(0, sig, (ncell, kmax))).astype(np.float32)
    w32 = np.float64(np.float32(1.0 / sig))
    L = 2.0 * np.eye(nlay)
    for i in range(1, nlay - 1):
        L[i, i - 1] = L[i, i + 1] = -1.0
    P = smooth ** 2 * L.T @ L + damp ** 2 * np.eye(nlay)
    assert np.linalg.matrix_rank(K.T @ K) == kmax < nlay          # the data alone leave two directions open
    cov = np.linalg.inv(K.T @ K * w32 ** 2 + P)
    vref = np.full(nlay, 3.5)
    rhs = cobs.astype(np.float64) - vref @ K.T                     # [ncell][kmax]
    mu = vref + (rhs @ K * w32 ** 2) @ cov                         # [ncell][nlay]
    return dict(ncell=ncell, kmax=kmax, nlay=nlay, sig=sig, smooth=smooth, damp=damp, K=K, cobs=cobs, rhs=rhs, mu=mu,
                sd=np.sqrt(np.diag(cov)))


def test_linear_gaussian_posterior_with_prior(ctx):
    """64 cells, 32 chains, 2000 burn-in and 8000 recorded steps of kind 0 in the box mu +- 6 sd, under test_linear_gaussian_posterior's
    bars: |mean - mu| <= 0.1 sd, |std / sd - 1| <= 0.1, R-hat < 1.05.  vref + dazim_column_lsq's solution and dazim_column_resolution's
    std_post on the same K table meet the same analytic mean and sd under the bars of their own tests (1e-6 of max(1, max |.|) per
    cell): the chains, the solve and the resolution call stand against each other."""
    pb = linear_problem()
    ncell, kmax, nlay, K, mu, sd = pb["ncell"], pb["kmax"], pb["nlay"], pb["K"], pb["mu"], pb["sd"]
    nx = ny = 10
    nz, nchain, nbin = nlay + 1, 32, 64
    sh = (ny - 2, nx - 2)
    vmin = (mu - 6 * sd).astype(np.float32)
    vmax = (mu + 6 * sd).astype(np.float32)
    vel0 = np.full((nz, ny, nx), 3.5, np.float32)
    wdat = np.full((kmax,) + sh, 1.0 / pb["sig"], np.float32)
    # the linearised side: the same K in every column of the table
    kern = np.ascontiguousarray(np.broadcast_to(K.T[:, :, None], (nlay, kmax, nx * ny)))
    x, ne, _ = ctx.column_lsq(nx, ny, nlay, kern, pb["rhs"].T.reshape((1, kmax) + sh).astype(np.float32), wdat, pb["smooth"], pb["damp"])
    res = ctx.column_resolution(nx, ny, nlay, kern, wdat, pb["smooth"], pb["damp"])
    assert ne == 0 and res["n_empty"] == 0 and res["n_failed"] == 0
    xr = (mu - 3.5).T                                              # [nlay][ncell]
    err = np.abs(x.reshape(nlay, ncell) - xr).max(axis=0) / np.maximum(1.0, np.abs(xr).max(axis=0))
    within("vref + column_lsq against the analytic posterior mean", err.max(), 1e-6)
    within("column_resolution's std_post against the analytic posterior sd", np.abs(res["std_post"].reshape(nlay, ncell) - sd[:, None]).max()
           / max(1.0, sd.max()), 1e-6)
    # the chains
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, 77, vel0, vmin.T.reshape((nlay,) + sh), vmax.T.reshape((nlay,) + sh),
                pb["cobs"].T.reshape((kmax,) + sh), wdat)
    mc.set_prior(pb["smooth"], pb["damp"])                         # vel0's knots: 3.5
    assert (mc.prior_state()["vref"] == np.float32(3.5)).all()
    for t in range(10000):
        v = mc.proposals().cpu().numpy()[:nlay].astype(np.float64)
        mc.step(K @ v, int(t >= 2000))
    r = mc.result()
    mean = r["mean"].reshape(nlay, ncell).T
    std = r["std"].reshape(nlay, ncell).T
    dmean = np.abs(mean - mu) / sd
    dstd = np.abs(std / sd - 1)
    dlin = np.abs(mean - (3.5 + x.reshape(nlay, ncell).T)) / res["std_post"].reshape(nlay, ncell).T
    print(f"\n[measured] |mean - mu| / sd max {dmean.max():.3f}; |std / sd - 1| max {dstd.max():.3f}; R-hat max {r['rhat'].max():.4f}; "
          f"acceptance {r['accept'].min():.3f}..{r['accept'].max():.3f}; against the library's own solve and std_post: |mean - (vref + x)| "
          f"/ std_post max {dlin.max():.3f}, std / std_post {(std / res['std_post'].reshape(nlay, ncell).T).min():.3f}.."
          f"{(std / res['std_post'].reshape(nlay, ncell).T).max():.3f}; posterior sd {sd.min():.4f}..{sd.max():.4f} km/s")
    assert dmean.max() <= 0.1
    assert dstd.max() <= 0.1
    assert r["rhat"].max() < 1.05
    mc.free()


MODES = [(kind, ntemp, noise) for kind in (0, 1) for ntemp in (1, 4) for noise in (0, 1)]


@pytest.mark.parametrize("kind,ntemp,noise", MODES)
def test_default_unchanged(ctx, kind, ntemp, noise):
    """set_prior(0, 0), after a prior had been set, is the handle that never saw the call: every field of state, result, cov_state,
    temper_state and noise_state of 60 + 20 steps of the dispersion forward model, in the bytes"""
    out = {}
    for name in ("plain", "zero"):
        mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, 4)
        if name == "zero":
            mc.set_prior(3.0, 2.0, truth[:-1, 1:-1, 1:-1] + np.float32(0.1))
            assert "q" in mc.prior_state()
            mc.set_prior(0.0, 0.0, np.full((mc.nlay, 3, 3), np.nan, np.float32))      # vref is not looked at
            assert mc.prior_state() == dict(smooth=0.0, damp=0.0)
        if kind == 1:
            mc.set_proposal(1)
        if ntemp > 1:
            mc.set_tempering(ntemp, 16.0, 1)
        if noise:
            mc.set_noise(2.0, 1.0)
        mc.run(depz, 3.0, periods, 60, 20)
        assert ctx.stat("mc.prior") == 0 and ctx.stat("mc.noise") == noise and ctx.stat("mc.proposal") == kind
        out[name] = everything(mc)
        out[name].update({"noise." + k: v for k, v in mc.noise_state().items() if isinstance(v, np.ndarray)})
        if noise:
            out[name].update({"noise_result." + k: v for k, v in mc.noise_result().items()})
        mc.free()
    assert out["plain"].keys() == out["zero"].keys()
    for k in out["plain"]:
        assert out["plain"][k].tobytes() == out["zero"][k].tobytes(), k


def test_dispersion_forward_with_and_without_prior(ctx):
    """6 x 6 cells, 7 knots (6 sampled), 8 periods, sigma_c 0.01, 16 chains, proposal 1, 500 + 500 steps, exact curves of a truth
    that is a smooth perturbation of the reference within 0.8 prior sd per knot; one seed with the prior (smooth 4, damp 4 about the
    reference) and without it: the median over cells and knots of std with / std without is below 1"""
    nx = ny = 8
    depz = np.array([0.0, 5.0, 10.0, 18.0, 28.0, 40.0, 60.0], np.float32)
    periods = np.array([6.0, 8.0, 10.0, 14.0, 18.0, 24.0, 30.0, 40.0])
    nz, kmax, nlay = len(depz), len(periods), len(depz) - 1
    smooth, damp = 4.0, 4.0
    L = 2.0 * np.eye(nlay)
    for i in range(1, nlay - 1):
        L[i, i - 1] = L[i, i + 1] = -1.0
    psd = np.sqrt(np.diag(np.linalg.inv(smooth ** 2 * L.T @ L + damp ** 2 * np.eye(nlay))))      # the prior's sd per knot
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    ref = np.broadcast_to((2.9 + 0.025 * depz)[:, None, None], (nz, ny, nx)).astype(np.float32)
    truth = ref.copy()
    for k in range(nlay):
        truth[k] += (0.8 * psd[k] * np.cos(0.5 * k) * np.sin(0.9 * ii + 0.5) * np.cos(0.7 * jj)).astype(np.float32)
    assert (np.abs(truth[:nlay] - ref[:nlay]) <= psd[:, None, None]).all() and np.abs(truth - ref).max() > 0.05
    pv, _, nf = ctx.depthkernel(truth, depz, periods, 3.0, kernels=False)
    assert nf == 0
    cobs = pv.reshape(kmax, ny, nx)[:, 1:-1, 1:-1].astype(np.float32)
    vmin, vmax = (ref[:nlay, 1:-1, 1:-1] - np.float32(0.5)), (ref[:nlay, 1:-1, 1:-1] + np.float32(0.5))
    wdat = np.full((kmax, ny - 2, nx - 2), 1.0 / 0.01, np.float32)
    out = {}
    for on in (False, True):
        mc = create(ctx, nx, ny, nz, kmax, 16, 100, 1, ref, vmin, vmax, cobs, wdat)
        mc.set_proposal(1)
        if on:
            mc.set_prior(smooth, damp)
        mc.run(depz, 3.0, periods, 500, 500)
        assert ctx.stat("mc.prior") == int(on)
        r = mc.result()
        t = truth[:nlay, 1:-1, 1:-1]
        out[on] = (r, ((r["q"][0] <= t) & (t <= r["q"][2])).mean(), ctx.stat("mc.step"), ctx.stat("mc"))
        mc.free()
    (r0, in0, s0, w0), (r1, in1, s1, w1) = out[False], out[True]
    ratio = np.median(r1["std"] / r0["std"])
    print(f"\n[measured] median std with / without the prior {ratio:.3f} (median std {np.median(r1['std']):.4f} against "
          f"{np.median(r0['std']):.4f} km/s; prior sd {psd.min():.3f}..{psd.max():.3f}); R-hat median / max {np.median(r1['rhat']):.3f} / "
          f"{r1['rhat'].max():.3f} with, {np.median(r0['rhat']):.3f} / {r0['rhat'].max():.3f} without; truth inside [p2.5, p97.5] "
          f"{in1:.3f} with, {in0:.3f} without; step kernels {s1:.3f} s with, {s0:.3f} s without of runs of {w1:.2f} s and {w0:.2f} s")
    assert ratio < 1


def test_refusals(ctx):
    nx = ny = 5
    nz, kmax = 4, 3
    sh = (ny - 2, nx - 2)
    args = dict(nx=nx, ny=ny, nz=nz, kmax=kmax, nchain=8, nbin=10, seed=1, vel0=np.full((nz, ny, nx), 3.5, np.float32),
                vmin=np.full((nz - 1,) + sh, 3.0, np.float32), vmax=np.full((nz - 1,) + sh, 4.0, np.float32),
                cobs=np.full((kmax,) + sh, 3.5, np.float32), wdat=np.ones((kmax,) + sh, np.float32), step=0.05, nadapt=50)
    mc = ctx.mc_create(**args)
    pv = np.full((kmax, mc.ncol), 3.4)
    vref = np.full((nz - 1,) + sh, 3.6, np.float32)

    def refused(call):
        with pytest.raises(dz.DazimError) as e:
            call()
        assert e.value.code == dz.DAZIM_E_BAD_ARG

    for bad in (-1.0, -1e-30, float("inf"), float("-inf"), float("nan")):
        refused(lambda: mc.set_prior(bad, 1.0))
        refused(lambda: mc.set_prior(1.0, bad))
        refused(lambda: mc.set_prior(bad, 0.0))
        refused(lambda: mc.set_prior(0.0, bad))
    for v in (np.inf, -np.inf, np.nan):
        bad = vref.copy()
        bad[1, 2, 0] = v
        refused(lambda: mc.set_prior(1.0, 1.0, bad))
        mc.set_prior(0.0, 0.0, bad)                            # the default does not look at vref
    refused(lambda: ctx.mc_create(**args, prior=(-1.0, 0.0)))
    assert mc.prior_state() == dict(smooth=0.0, damp=0.0)
    f, d = dz._ptr(np.zeros((nz - 1,) + sh, np.float32)), dz._ptr(np.zeros(mc.ncol))
    for arrs in ((f, None), (None, d)):                        # an array with the prior off
        assert ctx.lib.dazim_mc_prior_state(ctx._h, mc._h, None, None, *arrs) == dz.DAZIM_E_BAD_ARG
    other = dz.Context(0)
    assert other.lib.dazim_mc_set_prior(other._h, mc._h, 1.0, 1.0, None) == dz.DAZIM_E_BAD_ARG
    assert other.lib.dazim_mc_prior_state(other._h, mc._h, None, None, None, None) == dz.DAZIM_E_BAD_ARG
    other.close()
    mc.set_prior(2.0, 0.0, vref)                               # one of the two may be 0
    mc.set_prior(0.0, 1.5)
    mc.set_tempering(2, 4.0, 1)                                # the other setters after it
    mc.set_proposal(1)
    mc.set_noise(2.0, 1.0)
    ps = mc.prior_state()
    assert (ps["smooth"], ps["damp"]) == (0.0, 1.5) and (ps["vref"] == np.float32(3.5)).all()
    mc.step(pv, 0)
    refused(lambda: mc.set_prior(1.0, 1.0))                    # after a step
    refused(lambda: mc.set_prior(0.0, 0.0))
    mc.step(pv, 1)
    q = mc.prior_state()["q"]                                  # the handle still works
    cur = mc.state()["cur"]
    assert np.array_equal(q, mc_prior_ref.prior_q(cur[:nz - 1], np.full((nz - 1, mc.ncol), 3.5, np.float32), 0.0, 1.5))
    assert (q > 0).all() and np.isfinite(mc.result()["mean"]).all()
    mc.free()
