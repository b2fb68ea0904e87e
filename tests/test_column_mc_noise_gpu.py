"""-m gpu: the hierarchical data-noise scale of the Monte-Carlo sampler (dazim_mc_set_noise).

The step with the energy X = 2 a log(b0 + chi2 / 2) against its NumPy restatement (tests/mc_ref.py, driven by
tests/mc_step_check.py) in both proposal kinds, tempered and not, with the noise record and the result; the unchanged default and
reproducibility; a linear problem whose posterior is a multivariate t; the dispersion forward model with data noisier than assumed;
and the refused calls."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_ref
from tests.mc_step_check import check_final, drive, ulps
from tests.test_column_mc_gpu import create, disp_setup, per_column
from tests.test_column_mc_temper_gpu import host_forward, step_problem
from tests.test_mc_noise_ref_cpu import NBIN, NBURN, NCHAIN, NSAMPLE, SEED, check_linear

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    dz.build()
    c = dz.Context(0)
    yield c
    c.close()


NADAPT, NREC = 3, 4
A0, B0 = 0.25, 0.5
# (nz, nchain, ntemp, nswap, kind): nburn.  Kind 0 crosses two adaptation points; kind 1 goes on to the adaptation point at which the
# rung-0 chains have given the 8 nlay states of the first factor, and one window beyond it (tests/test_column_mc_temper_gpu.py)
SHAPES = {
    "untempered": ((6, 32, 1, 1, 0), 8),
    "odd0": ((6, 6, 3, 2, 0), 8),
    "odd1": ((6, 6, 3, 2, 1), 25),
    "plain1": ((12, 32, 4, 1, 1), 16),
    "one_group": ((3, 8, 8, 1, 0), 8),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_noise_step_against_numpy(ctx, shape):
    """every step restated from the library's own state, ladder, proposals, cov_state and noise_state: decisions, cur, chi2, sums,
    hist, best, the swap counters, nsum and ncnt bit for bit, proposals within one fp32 ulp, lam_mean and lam_std equal to the
    restatement's or one fp32 ulp from it.  a0 = 0.25 gives the one-period cell a = 0.75: lam_std NaN; the cell without data 0."""
    (nz, nchain, ntemp, nswap, kind), nburn = SHAPES[shape]
    rng, nx, ny, kmax, vel0, vmin, vmax, cobs, wdat = step_problem(nz)
    nbin, seed, tmax = 20, 0x1234_5678_9ABC, 16.0
    ncell, ncs = 16, 15
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, 0.05, NADAPT)
    if shape == "odd1":                         # the setters in either order
        mc.set_noise(A0, B0)
    if kind == 1:
        mc.set_proposal(1)
    if ntemp > 1:
        mc.set_tempering(ntemp, tmax, nswap)
    if shape != "odd1":
        mc.set_noise(2.0, 1.0)                  # a second call replaces the prior
        mc.set_noise(A0, B0)
    ns = mc.noise_state()
    assert (ns["a0"], ns["b0"]) == (A0, B0) and not ns["nsum"].any() and not ns["ncnt"].any()
    assert ns["nsum"].shape == (2, mc.ncol) and ns["ncnt"].shape == (mc.ncol,)
    lo, hi = per_column(vmin.astype(np.float64), mc), per_column(vmax.astype(np.float64), mc)
    cb, wd = per_column(cobs, mc), per_column(wdat, mc)
    # (without swaps a moved state is an accepted proposal: the decisions themselves)
    run = drive(mc, lambda t: host_forward(rng, cb, t, nswap), nburn, NREC, NADAPT, lo, hi, cb, wd, nbin, seed, moved=ntemp == 1)
    got, gtp, gcov, gns, seen, ndec = run["got"], run["gtp"], run["gcov"], run["gns"], run["seen"], run["ndec"]
    hot = (np.arange(mc.ncol) % nchain) % ntemp != 0
    assert not gns["nsum"][:, hot].any() and not gns["ncnt"][hot].any()              # the columns of the hot chains stay 0
    assert 0 < gns["ncnt"].sum() <= NREC * ncs * (nchain // ntemp) and gns["ncnt"].max() == NREC
    assert ndec > 0 and (got["scale"] != np.float32(0.05)).any()
    if ntemp > 1:
        assert all(seen[k] > 0 for k in seen), seen                                  # every case of the swap rule
        assert 0 < gtp["swap_acc"].sum() < gtp["swap_try"].sum()
    if kind == 1:
        assert (gcov["cov_set"] == 1).all()
    # the result against its restatement
    r = mc.noise_result()
    e = mc_ref.result(gns, wdat.reshape(kmax, ncell), mc._cells, ncell, nchain, ntemp)
    assert np.array_equal(r["ndata"].ravel(), e["ndata"])
    one, none = 0, 6                            # step_problem's cell with one weighted period, and its cell without data
    assert e["ndata"][one] == 1 and e["ndata"][none] == 0
    assert np.isnan(r["lam_std"].ravel()[one]) and np.isfinite(r["lam_mean"].ravel()[one]) and r["lam_mean"].ravel()[one] > 0
    assert r["lam_mean"].ravel()[none] == 0 and r["lam_std"].ravel()[none] == 0
    for k in ("lam_mean", "lam_std"):
        a, b = r[k].ravel(), e[k]
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin) and fin.sum() >= 14, k
        assert ulps(a[fin], b[fin]).max() <= 1, k
    # the Vs statistics are those of the recorded states, as without the mode
    check_final(mc, got, vmin, vmax, vel0, ntemp, NREC, nbin, roots=False)
    print(f"\n[measured] {shape}: swap cases {seen}; recorded noise states {gns['ncnt'].sum()}; lam_mean "
          f"{np.nanmin(r['lam_mean'][r['ndata'] > 0]):.3f}..{np.nanmax(r['lam_mean']):.3f}")
    mc.free()


def everything(mc):
    out = {"result." + k: v for k, v in mc.result().items()}
    out.update({"state." + k: v for k, v in mc.state().items() if k != "step"})
    out.update({"cov." + k: v for k, v in mc.cov_state().items() if k != "kind"})
    out.update({"temper." + k: v for k, v in mc.temper_state().items() if isinstance(v, np.ndarray)})
    return out


def test_default_unchanged_and_reproducible(ctx):
    """set_noise(0, ..) is the untouched handle in every field of state / result (kind 1, 4 rungs, 120 + 40 steps of the dispersion
    forward model); two runs with the mode on and one seed give the same bytes, and other ones than the default"""
    res, noise = {}, {}
    for name in ("plain", "zero", "a", "b"):
        mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, 4)
        mc.set_proposal(1)
        if name == "zero":
            mc.set_noise(2.0, 1.0)                            # and back to the default; b0 is not looked at
            mc.set_noise(0.0, -1.0)
            assert mc.noise_state() == dict(a0=0.0, b0=0.0)
        elif name != "plain":
            mc.set_noise(2.0, 1.0)
        mc.set_tempering(4, 16.0, 1)
        mc.run(depz, 3.0, periods, 120, 40)
        assert ctx.stat("mc.noise") == (1 if name in "ab" else 0)
        res[name] = everything(mc)
        if name in "ab":
            noise[name] = dict(mc.noise_result(), **{k: v for k, v in mc.noise_state().items() if isinstance(v, np.ndarray)})
        mc.free()
    assert res["plain"].keys() == res["zero"].keys()
    for k in res["plain"]:
        assert res["plain"][k].tobytes() == res["zero"][k].tobytes(), k
    for k in res["a"]:
        assert res["a"][k].tobytes() == res["b"][k].tobytes(), k
    for k in noise["a"]:
        assert noise["a"][k].tobytes() == noise["b"][k].tobytes(), k
    assert noise["a"]["ncnt"].sum() > 0 and (noise["a"]["lam_mean"] > 0).all()
    assert not np.array_equal(res["a"]["state.cur"], res["plain"]["state.cur"])
    assert not np.array_equal(res["a"]["result.mean"], res["plain"]["result.mean"])


def test_linear_student_t_posterior(ctx):
    """c = K v (fp64, host): 16 cells, 12 periods, 4 knots, 32 chains, w = 1 / 0.02 against data noise 0.06, a0 = 2, b0 = 1, 2000
    burn-in and 8000 recorded steps against the multivariate t (tests/mc_ref.linear_problem) under the bars of
    test_linear_gaussian_posterior; lam_mean and lam_std, second-moment estimates from the same states, within 10 % too.  The same
    run with the mode off is printed beside it: its std is the too-small fixed-sigma one."""
    pb = mc_ref.linear_problem()
    ncell, kmax, nlay, K = pb["ncell"], pb["kmax"], pb["nlay"], pb["K"]
    nx = ny = 6
    nz = nlay + 1
    sh = (ny - 2, nx - 2)
    vel0 = np.full((nz, ny, nx), 3.5, np.float32)
    wdat = np.full((kmax,) + sh, pb["w"], np.float32)
    out = {}
    for on in (True, False):
        mc = create(ctx, nx, ny, nz, kmax, NCHAIN, NBIN, SEED, vel0, pb["vmin"].T.reshape((nlay,) + sh),
                    pb["vmax"].T.reshape((nlay,) + sh), pb["cobs"].T.reshape((kmax,) + sh), wdat)
        if on:
            mc.set_noise(pb["a0"], pb["b0"])
        for t in range(NBURN + NSAMPLE):
            v = mc.proposals().cpu().numpy()[:nlay].astype(np.float64)
            mc.step(K @ v, int(t >= NBURN))
        out[on] = (mc.result(), mc.noise_result() if on else None)
        mc.free()
    r, nr = out[True]
    std_off = out[False][0]["std"].reshape(nlay, ncell).T
    print(f"\n[measured] mode off, same problem and seed: std / fixed-sigma analytic {(std_off / pb['sd_fixed']).min():.3f}.."
          f"{(std_off / pb['sd_fixed']).max():.3f}; std / Student-t analytic {(std_off / pb['sd']).min():.3f}.."
          f"{(std_off / pb['sd']).max():.3f}")
    assert (nr["ndata"] == kmax).all()
    check_linear(pb, r["mean"].reshape(nlay, ncell).T, r["std"].reshape(nlay, ncell).T, r["rhat"], nr["lam_mean"].ravel(),
                 nr["lam_std"].ravel(), "library, mode on")


def test_dispersion_forward_noisy_data(ctx):
    """disp_setup's 6 x 6 cells with noise of std 0.03 added to the curves against w = 1 / 0.01, proposal 1, 1000 + 1000 steps: the
    median lam_mean is above 1 and the median Vs std grows against the same run with the mode off"""
    nx = ny = 8
    mc, truth, depz, periods = disp_setup(ctx, nx, ny, 0.01)
    mc.free()
    # disp_setup's handle again with noise on its exact curves
    nz, kmax = len(depz), len(periods)
    pv, _, nf = ctx.depthkernel(truth, depz, periods, 3.0, kernels=False)
    cobs = pv.reshape(kmax, ny, nx)[:, 1:-1, 1:-1] + np.random.default_rng(12).normal(0, 0.03, (kmax, ny - 2, nx - 2))
    mean = truth[:-1].mean(axis=(1, 2))
    vmin = np.broadcast_to((mean - 0.5)[:, None, None], (nz - 1, ny - 2, nx - 2)).astype(np.float32)
    vmax = np.broadcast_to((mean + 0.5)[:, None, None], (nz - 1, ny - 2, nx - 2)).astype(np.float32)
    wdat = np.full((kmax, ny - 2, nx - 2), 1.0 / 0.01, np.float32)
    out = {}
    for on in (False, True):
        mc = create(ctx, nx, ny, nz, kmax, 16, 100, 1, truth, vmin, vmax, cobs.astype(np.float32), wdat)
        mc.set_proposal(1)
        if on:
            mc.set_noise(2.0, 1.0)
        mc.run(depz, 3.0, periods, 1000, 1000)
        out[on] = (mc.result(), mc.noise_result() if on else None, ctx.stat("mc.step"), ctx.stat("mc"))
        mc.free()
    (r0, _, s0, w0), (r1, nr, s1, w1) = out[False], out[True]
    ratio = np.median(r1["std"] / r0["std"])
    lam = nr["lam_mean"]
    print(f"\n[measured] data noise 0.03 against sigma_c 0.01: lam_mean min / quartiles / max {lam.min():.2f} "
          f"{np.percentile(lam, 25):.2f} {np.median(lam):.2f} {np.percentile(lam, 75):.2f} {lam.max():.2f}; lam_std median "
          f"{np.median(nr['lam_std']):.2f}; median Vs std on / off {ratio:.2f} (median std {np.median(r1['std']):.4f} against "
          f"{np.median(r0['std']):.4f} km/s); R-hat median {np.median(r1['rhat']):.3f} on, {np.median(r0['rhat']):.3f} off; step "
          f"kernels {s1:.3f} s on, {s0:.3f} s off of runs of {w1:.2f} s and {w0:.2f} s")
    assert (nr["ndata"] == 8).all()
    assert np.median(lam) > 1
    assert ratio > 1


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

    for a0 in (-1.0, -1e-30, float("inf"), float("-inf"), float("nan")):
        refused(lambda: mc.set_noise(a0, 1.0))
    for b0 in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        refused(lambda: mc.set_noise(2.0, b0))
        mc.set_noise(0.0, b0)                                  # a0 = 0 does not look at b0
    refused(lambda: ctx.mc_create(**args, noise=(2.0, 0.0)))
    assert mc.noise_state() == dict(a0=0.0, b0=0.0)
    n2, n1 = dz._ptr(np.zeros((2, mc.ncol))), dz._ptr(np.zeros(mc.ncol, np.int64))
    for arrs in ((n2, None), (None, n1)):                      # an array with the mode off
        assert ctx.lib.dazim_mc_noise_state(ctx._h, mc._h, None, None, *arrs) == dz.DAZIM_E_BAD_ARG
    refused(mc.noise_result)                                   # the mode off
    other = dz.Context(0)
    assert other.lib.dazim_mc_set_noise(other._h, mc._h, 2.0, 1.0) == dz.DAZIM_E_BAD_ARG
    assert other.lib.dazim_mc_noise_state(other._h, mc._h, None, None, None, None) == dz.DAZIM_E_BAD_ARG
    f, i = dz._ptr(np.zeros(sh, np.float32)), dz._ptr(np.zeros(sh, np.int32))
    assert other.lib.dazim_mc_noise_result(other._h, mc._h, f, f, i) == dz.DAZIM_E_BAD_ARG
    other.close()
    mc.set_noise(2.0, 1.0)
    mc.set_tempering(2, 4.0, 1)                                # the other setters after it
    mc.set_proposal(1)
    ns = mc.noise_state()
    assert (ns["a0"], ns["b0"]) == (2.0, 1.0)
    refused(mc.noise_result)                                   # before the first recorded step
    mc.step(pv, 0)
    refused(mc.noise_result)
    refused(lambda: mc.set_noise(2.0, 1.0))                    # after a step
    refused(lambda: mc.set_noise(0.0, 1.0))
    mc.step(pv, 1)
    r = mc.noise_result()                                      # the handle still works
    assert (r["ndata"] == kmax).all() and (r["lam_mean"] > 0).all() and (r["lam_std"] > 0).all()
    assert (mc.noise_state()["ncnt"].reshape(-1, 8)[:, ::2] == 1).all()
    mc.free()
