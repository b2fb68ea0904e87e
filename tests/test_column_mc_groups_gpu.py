"""-m gpu: one noise scale per group of periods and typed data in the Monte-Carlo sampler (dazim_mc_set_noise_groups,
dazim_mc_set_segments).

The step with the energy X = sum_g 2 a_g log(b0_g + chi2_g / 2) against its NumPy restatement (tests/mc_ref.py, driven by
tests/mc_step_check.py) at the shapes of tests/test_column_mc_noise_gpu.py with two interleaved and four contiguous groups, and at two
of them with the smoothness prior beside the groups; one group, all-zero a0 and a repeated seed as
bytes; the linear problem of tests/test_mc_groups_ref_cpu.py through the library; dazim_mc_run's typed forward call against a hand
loop; four wave types against Rayleigh phase alone on exact curves; noisier Love data; and the refused calls."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_groups_ref as gr
from tests import mc_ref
from tests.mc_step_check import check_final, drive, ulps
from tests.test_column_mc_gpu import create, disp_setup, per_column
from tests.test_column_mc_noise_gpu import NADAPT, NREC, SHAPES, everything
from tests.test_column_mc_temper_gpu import host_forward, step_problem
from tests.test_mc_groups_ref_cpu import SEED, check_linear_groups, linear_reference
from tests.test_mc_noise_ref_cpu import NBIN, NBURN, NCHAIN, NSAMPLE
from tests.typed_kernels_ref import DEPZ, LC, LG, RC, RG, SUBLAYERS, common_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    dz.build()
    c = dz.Context(0)
    yield c
    c.close()


# the group of step_problem's period 3, the one weighted period of its cell 0, has a0 = 0.25: a = 0.75 there, lam_std NaN
GROUPS = {2: (np.arange(8) % 2, [0.5, 0.25], [0.5, 1.0]), 4: (np.arange(8) // 2, [0.5, 0.25, 0.75, 1.0], [0.5, 1.0, 0.75, 2.0])}


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_groups_step_against_numpy(ctx, shape, G):
    """decisions, cur, chi2, chi2g, sums, hist, best, the swap counters, nsum and ncnt bit for bit, proposals within one fp32 ulp,
    lam_mean and lam_std equal to the restatement's or one fp32 ulp from it; cell 0 has one weighted period: its group's lam_std is
    NaN (a = 0.75) and its other groups, without data, give 0; the cell without data gives 0 everywhere"""
    (nz, nchain, ntemp, nswap, kind), nburn = SHAPES[shape]
    rng, nx, ny, kmax, vel0, vmin, vmax, cobs, wdat = step_problem(nz)
    grp, a0, b0 = GROUPS[G]
    nbin, seed, tmax = 20, 0x1234_5678_9ABC, 16.0
    ncell, ncs = 16, 15
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, 0.05, NADAPT)
    if shape == "odd1":                         # the setters in either order
        mc.set_noise_groups(grp, a0, b0)
    if kind == 1:
        mc.set_proposal(1)
    if ntemp > 1:
        mc.set_tempering(ntemp, tmax, nswap)
    if shape != "odd1":
        mc.set_noise(2.0, 1.0)                  # a later call replaces the mode
        mc.set_noise_groups(grp, a0, b0)
    gs = mc.noise_groups_state()
    assert gs["ngroup"] == G and np.array_equal(gs["group_of_period"], grp)
    assert np.array_equal(gs["a0"], np.float32(a0)) and np.array_equal(gs["b0"], np.float32(b0))
    assert gs["chi2g"].shape == (G, mc.ncol) and np.isinf(gs["chi2g"]).all() and not gs["nsum"].any() and not gs["ncnt"].any()
    assert mc.noise_state() == dict(a0=0.0, b0=0.0)                  # the single scale is not what is on
    lo, hi = per_column(vmin.astype(np.float64), mc), per_column(vmax.astype(np.float64), mc)
    cb, wd = per_column(cobs, mc), per_column(wdat, mc)
    run = drive(mc, lambda t: host_forward(rng, cb, t, nswap), nburn, NREC, NADAPT, lo, hi, cb, wd, nbin, seed, moved=ntemp == 1)
    got, gtp, gcov, ggs, seen = run["got"], run["gtp"], run["gcov"], run["gns"], run["seen"]
    hot = (np.arange(mc.ncol) % nchain) % ntemp != 0
    assert not ggs["nsum"][:, :, hot].any() and not ggs["ncnt"][hot].any()
    assert 0 < ggs["ncnt"].sum() <= NREC * ncs * (nchain // ntemp) and ggs["ncnt"].max() == NREC
    assert run["ndec"] > 0 and (got["scale"] != np.float32(0.05)).any()
    assert run["ninf_group"] > 0                                     # states with a root missing in exactly one group
    if ntemp > 1:
        assert all(seen[k] > 0 for k in mc_ref.BRANCHES), seen      # every case of the swap rule
        assert 0 < gtp["swap_acc"].sum() < gtp["swap_try"].sum()
    if kind == 1:
        assert (gcov["cov_set"] == 1).all()
    r = mc.noise_groups_result()
    e = gr.result(ggs, wdat.reshape(kmax, ncell), mc._cells, ncell, nchain, ntemp)
    nd = r["ndata"].reshape(G, ncell)
    assert np.array_equal(nd, e["ndata"]) and np.array_equal(nd.sum(axis=0), (wdat.reshape(kmax, ncell) != 0).sum(axis=0))
    one, none, g3 = 0, 6, int(grp[3])
    lm, ls = r["lam_mean"].reshape(G, ncell), r["lam_std"].reshape(G, ncell)
    assert nd[g3, one] == 1 and nd[:, one].sum() == 1 and not nd[:, none].any()
    assert np.isnan(ls[g3, one]) and np.isfinite(lm[g3, one]) and lm[g3, one] > 0
    assert not np.delete(lm[:, one], g3).any() and not np.delete(ls[:, one], g3).any()      # groups without data in a sampled cell
    assert not lm[:, none].any() and not ls[:, none].any()
    for k, a in (("lam_mean", lm), ("lam_std", ls)):
        fin = np.isfinite(e[k])
        assert np.array_equal(np.isfinite(a), fin) and fin[:, mc._cells].mean() > 0.5, k
        assert ulps(a[fin], e[k][fin]).max() <= 1, k
    check_final(mc, got, vmin, vmax, vel0, ntemp, NREC, nbin, roots=False)
    print(f"\n[measured] {shape}, {G} groups: swap cases {seen}; recorded noise states {ggs['ncnt'].sum()}; states with one group at "
          f"+inf {run['ninf_group']}; lam_mean {np.nanmin(lm[nd > 0]):.3f}..{np.nanmax(lm):.3f}")
    mc.free()


@pytest.mark.parametrize("shape,G", [("untempered", 4), ("odd1", 2)])
def test_groups_with_prior_step_against_numpy(ctx, shape, G):
    """k_mc_step with several groups and the prior together, step by step: everything tests/mc_step_check.drive compares (state,
    ladder, covariance sums, chi2g, nsum, ncnt and q bit for bit, q against Q of the new states, the factor, the proposals) with
    GROUPS' priors and smooth 3, damp 4 about a random reference inside the boxes, as in test_prior_step_against_numpy; some
    decisions come out otherwise than the energies alone would have made them, some states have exactly one group at +inf, and the
    ladder meets every case of the swap rule (tests/test_mc_groups_ref_cpu.py reaches these counts with the restatement alone)"""
    (nz, nchain, ntemp, nswap, kind), nburn = SHAPES[shape]
    rng, nx, ny, kmax, vel0, vmin, vmax, cobs, wdat = step_problem(nz)
    grp, a0, b0 = GROUPS[G]
    nbin, seed, tmax = 20, 0x1234_5678_9ABC, 16.0
    vref = (vmin + np.random.default_rng(nz).uniform(0.1, 0.9, vmin.shape) * (vmax - vmin)).astype(np.float32)
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, 0.05, NADAPT)
    mc.set_noise_groups(grp, a0, b0)
    if kind == 1:
        mc.set_proposal(1)
    if ntemp > 1:
        mc.set_tempering(ntemp, tmax, nswap)
    mc.set_prior(3.0, 4.0, vref)
    lo, hi = per_column(vmin.astype(np.float64), mc), per_column(vmax.astype(np.float64), mc)
    cb, wd, vr = per_column(cobs, mc), per_column(wdat, mc), per_column(vref, mc)
    run = drive(mc, lambda t: host_forward(rng, cb, t, nswap), nburn, NREC, NADAPT, lo, hi, cb, wd, nbin, seed, moved=ntemp == 1, vref=vr)
    print(f"\n[measured] {shape}, {G} groups and the prior: decisions {run['ndec']} accepted, {run['ndiff_dec']} other than the energies "
          f"alone, {run['ndiff_swap']} swap rules; states with one group at +inf {run['ninf_group']}; swap cases {run['seen']}")
    assert run["gns"]["ngroup"] == G and run["gpr"] is not None and run["gns"]["ncnt"].sum() > 0
    assert run["ndec"] > 0 and run["ndiff_dec"] > 0
    assert run["ninf_group"] > 0
    if ntemp > 1:
        assert all(run["seen"][k] > 0 for k in mc_ref.BRANCHES), run["seen"]
    if kind == 1:
        assert (run["gcov"]["cov_set"] == 1).all()
    mc.free()


def groups_everything(mc):
    out = everything(mc)
    out.update({"groups." + k: np.asarray(v) for k, v in mc.noise_groups_state().items()})
    if out["groups.ngroup"] > 0:
        out.update({"groups_result." + k: v for k, v in mc.noise_groups_result().items()})
    out.update({"prior." + k: np.asarray(v) for k, v in mc.prior_state().items()})
    return out


def test_equivalences(ctx):
    """kind 1, 4 rungs, 120 + 40 steps of the dispersion forward model: set_noise_groups with one group is set_noise in every field
    of state, result and noise result; all-zero a0 is the untouched handle; two runs with two groups and one seed give the same
    bytes, and other ones than one group"""
    res, noise = {}, {}
    grp2 = np.arange(8) % 2
    for name in ("plain", "zero", "noise", "one", "a", "b"):
        mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, 4)
        mc.set_proposal(1)
        if name == "zero":
            mc.set_noise_groups(grp2, [2.0, 1.5], [1.0, 1.0])
            mc.set_noise_groups(grp2, [0.0, 0.0], [-1.0, float("nan")])      # b0 is not looked at
            assert mc.noise_groups_state() == dict(ngroup=0) and mc.noise_state() == dict(a0=0.0, b0=0.0)
        elif name == "noise":
            mc.set_noise(2.0, 1.0)
        elif name == "one":
            mc.set_noise_groups(np.zeros(8, np.int32), [2.0], [1.0])
        elif name in "ab":
            mc.set_noise_groups(grp2, [2.0, 1.5], [1.0, 0.5])
        mc.set_tempering(4, 16.0, 1)
        mc.run(depz, 3.0, periods, 120, 40)
        assert ctx.stat("mc.noise") == dict(plain=0, zero=0, noise=1, one=1, a=2, b=2)[name]
        assert ctx.stat("mc.noise_groups") == dict(plain=0, zero=0, noise=1, one=1, a=2, b=2)[name]
        res[name] = groups_everything(mc)
        if name in ("noise", "one"):
            noise[name] = dict(mc.noise_result(), **{k: v for k, v in mc.noise_state().items() if isinstance(v, np.ndarray)})
        mc.free()
    for x, y in (("plain", "zero"), ("noise", "one"), ("a", "b")):
        assert res[x].keys() == res[y].keys()
        for k in res[x]:
            assert res[x][k].tobytes() == res[y][k].tobytes(), (x, y, k)
    for k in noise["noise"]:
        assert noise["noise"][k].tobytes() == noise["one"][k].tobytes(), k
    # one group's records in the groups' layout are the single scale's own
    assert res["one"]["groups.nsum"].tobytes() == noise["one"]["nsum"].tobytes()
    assert res["one"]["groups.chi2g"].tobytes() == res["one"]["state.chi2"].tobytes()
    for k in ("lam_mean", "lam_std", "ndata"):
        assert res["one"]["groups_result." + k].tobytes() == noise["one"][k].tobytes(), k
    assert res["a"]["groups.ncnt"].sum() > 0 and (res["a"]["groups_result.lam_mean"] > 0).all()
    assert not np.array_equal(res["a"]["state.cur"], res["one"]["state.cur"])
    assert not np.array_equal(res["a"]["state.cur"], res["plain"]["state.cur"])


def test_linear_two_groups(ctx):
    """the linear problem of tests/test_mc_groups_ref_cpu.py (16 cells, 2 knots, 2 groups x 12 periods, the second at 3 x the assumed
    noise, 32 chains, 2000 + 8000 steps) through the library, against quadrature over the box under check_linear's bars per group"""
    pb, ref, sd_fixed = linear_reference()
    ncell, kmax, nlay, K = pb["ncell"], pb["kmax"], pb["nlay"], pb["K"]
    nx = ny = 6
    nz = nlay + 1
    sh = (ny - 2, nx - 2)
    vel0 = np.full((nz, ny, nx), 3.5, np.float32)
    wdat = np.full((kmax,) + sh, pb["w"], np.float32)
    mc = create(ctx, nx, ny, nz, kmax, NCHAIN, NBIN, SEED, vel0, pb["vmin"].T.reshape((nlay,) + sh), pb["vmax"].T.reshape((nlay,) + sh),
                pb["cobs"].T.reshape((kmax,) + sh), wdat)
    mc.set_noise_groups(pb["grp"], pb["a0"], pb["b0"])
    for t in range(NBURN + NSAMPLE):
        v = mc.proposals().cpu().numpy()[:nlay].astype(np.float64)
        mc.step(K @ v, int(t >= NBURN))
    r, nr = mc.result(), mc.noise_groups_result()
    mc.free()
    assert (nr["ndata"] == kmax // 2).all()
    check_linear_groups(pb, ref, sd_fixed, r["mean"].reshape(nlay, ncell).T, r["std"].reshape(nlay, ncell).T, r["rhat"],
                        nr["lam_mean"].reshape(2, ncell), nr["lam_std"].reshape(2, ncell), "library")


T3 = np.array([6.0, 12.0, 20.0])
SEG4 = [RC + (T3,), RG + (T3,), LC + (T3,), LG + (T3,)]


def typed_handle(ctx, segments, nchain=8, seed=3, half=0.3):
    """tests/typed_kernels_ref's model on 5 x 5 nodes (every curve complete): the data are its own typed curves at the inner cells"""
    vel = common_model(5, 5, ended=False)
    nz, ny, nx = vel.shape
    pv, _, nf = ctx.dispersion_kernels_typed(vel, DEPZ, segments, SUBLAYERS, kernels=False)
    K = pv.shape[0]
    cobs = pv.reshape(K, ny, nx)[:, 1:-1, 1:-1].astype(np.float32)
    wdat = np.where(cobs != 0, np.float32(1.0 / 0.02), np.float32(0)).astype(np.float32)
    assert (wdat != 0).mean() > 0.9
    inner = vel[:-1, 1:-1, 1:-1]
    mc = create(ctx, nx, ny, nz, K, nchain, 20, seed, vel, inner - np.float32(half), inner + np.float32(half), cobs, wdat, 0.05, 3)
    return mc, vel, np.concatenate([s[2] for s in segments])


@pytest.mark.parametrize("modes", ["plain", "all"])
def test_typed_run_is_the_hand_loop(ctx, modes):
    """dazim_mc_run on a handle with four segments of 3 periods against proposals() -> dispersion_kernels_typed(kernels=False) ->
    step() on a second handle, 6 + 4 steps of 8 chains: every field of state and result byte for byte; `all`: kind 1, 4 rungs, the
    smoothness prior and four noise groups on, none of which looks at a period's type"""
    nburn, nrec = 6, 4
    out = []
    for hand in (False, True):
        mc, vel, periods = typed_handle(ctx, SEG4)
        if modes == "all":
            mc.set_proposal(1)
            mc.set_tempering(4, 8.0, 1)
            mc.set_prior(0.5, 0.2)
            mc.set_noise_groups(np.repeat(np.arange(4), 3), [2.0] * 4, [1.0] * 4)
        mc.set_segments(SEG4)
        nf_run = nf_loop = 0
        if hand:
            for t in range(nburn + nrec):
                prop = mc.proposals()
                pv, _, nf = ctx.dispersion_kernels_typed(prop.reshape(mc.nz, 1, mc.ncol), DEPZ, SEG4, SUBLAYERS, kernels=False)
                nf_loop += nf
                mc.step(pv, int(t >= nburn))
        else:
            nf_run = mc.run(DEPZ, SUBLAYERS, periods, nburn, nrec)
            assert ctx.stat("mc.steps") == nburn + nrec and ctx.stat("mc.disp") > 0 and ctx.stat("mc.step") > 0
            assert ctx.stat("mc.noise_groups") == (4 if modes == "all" else 0)
        out.append(groups_everything(mc))
        assert mc.state()["step"] == nburn + nrec
        mc.free()
    assert out[0].keys() == out[1].keys()
    for k in out[0]:
        assert out[0][k].tobytes() == out[1][k].tobytes(), k
    assert np.isfinite(out[0]["state.chi2"]).mean() > 0.5 and (out[0]["state.cur"] != out[0]["state.cur"][:, :1]).any()


def test_rayleigh_phase_segment_is_the_default(ctx):
    """set_segments([(2, 0, t)]) against no call, 30 + 20 steps of dazim_mc_run: the same bytes; and back from four segments"""
    res = []
    for name in ("none", "rc"):
        mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, 4)
        if name == "rc":
            mc.set_segments([RC + (4,), LC + (4,)])
            mc.set_segments([RC + (periods,)])
        mc.run(depz, 3.0, periods, 30, 20)
        res.append(everything(mc))
        mc.free()
    for k in res[0]:
        assert res[0][k].tobytes() == res[1][k].tobytes(), k


NOISE_LOVE = 0.03      # 3 sigma_c
_RUNS = {}


def typed_runs(ctx):
    """disp_setup's 6 x 6 cells and periods with the exact curves of its true model in four wave types, proposal 1, 250 + 400 steps
    and one seed: Rayleigh phase alone, the four types, and the four types with noise of 3 sigma_c on the Love segments and one noise
    scale per type.  Computed once for the two tests below"""
    if _RUNS:
        return _RUNS
    nx = ny = 8
    sigma = 0.01
    mc, truth, depz, periods = disp_setup(ctx, nx, ny, sigma)
    mc.free()
    nz, kmax = len(depz), len(periods)
    seg4 = [RC + (periods,), RG + (periods,), LC + (periods,), LG + (periods,)]
    pv, _, nf = ctx.dispersion_kernels_typed(truth, depz, seg4, 3.0, kernels=False)
    assert nf == 0 and (pv != 0).all()
    exact = pv.reshape(4 * kmax, ny, nx)[:, 1:-1, 1:-1]
    noisy = exact.copy()
    noisy[2 * kmax:] += np.random.default_rng(12).normal(0, NOISE_LOVE, noisy[2 * kmax:].shape)
    mean = truth[:-1].mean(axis=(1, 2))
    vmin = np.broadcast_to((mean - 0.5)[:, None, None], (nz - 1, ny - 2, nx - 2)).astype(np.float32)
    vmax = np.broadcast_to((mean + 0.5)[:, None, None], (nz - 1, ny - 2, nx - 2)).astype(np.float32)
    for name, segs, cobs in (("rc", seg4[:1], exact[:kmax]), ("four", seg4, exact), ("noisy", seg4, noisy)):
        K = kmax * len(segs)
        mc = create(ctx, nx, ny, nz, K, 16, 100, 1, truth, vmin, vmax, cobs.astype(np.float32), np.full((K, ny - 2, nx - 2), 1.0 / sigma,
                                                                                                         np.float32))
        mc.set_proposal(1)
        mc.set_segments(segs)
        if name == "noisy":
            mc.set_noise_groups(np.repeat(np.arange(4), kmax), [2.0] * 4, [1.0] * 4)
        nr = mc.run(depz, 3.0, np.concatenate([s[2] for s in segs]), 250, 400)
        _RUNS[name] = dict(r=mc.result(), nr=mc.noise_groups_result() if name == "noisy" else None, no_root=nr,
                           sec=(ctx.stat("mc"), ctx.stat("mc.disp"), ctx.stat("mc.step")), rhat=float(np.median(mc.result()["rhat"])))
        mc.free()
    _RUNS["truth"] = truth[:-1, 1:-1, 1:-1]
    return _RUNS


def test_four_types_recover_better_than_rayleigh_phase(ctx):
    """the mean posterior std over cells and knots with four types is below that with Rayleigh phase alone, and the truth stays
    inside [p2.5, p97.5] for 0.9 of (cell, knot), the bar of tests/test_column_mc_gpu.py's dispersion test"""
    runs = typed_runs(ctx)
    t = runs["truth"]
    fig = {}
    for name in ("rc", "four"):
        r = runs[name]["r"]
        fig[name] = (float(r["std"].mean()), float(((r["q"][0] <= t) & (t <= r["q"][2])).mean()))
        print(f"\n[measured] {name}: mean posterior std {fig[name][0]:.4f} km/s; truth inside [p2.5, p97.5] for {fig[name][1]:.3f} of "
              f"(cell, knot); R-hat median {runs[name]['rhat']:.3f}; no root {runs[name]['no_root']}; run, dispersion, steps "
              f"{runs[name]['sec'][0]:.2f} {runs[name]['sec'][1]:.2f} {runs[name]['sec'][2]:.3f} s")
    assert fig["four"][0] < fig["rc"][0]
    assert fig["four"][1] >= 0.9 and fig["rc"][1] >= 0.9


def test_noise_scale_per_type(ctx):
    """noise of 3 sigma_c on the Love segments only: the median lam_mean of the two Love groups exceeds that of the two Rayleigh ones"""
    nr = typed_runs(ctx)["noisy"]["nr"]
    med = np.median(nr["lam_mean"].reshape(4, -1), axis=1)
    print(f"\n[measured] median lam_mean per type (Rc, Rg, Lc, Lg): {med[0]:.2f} {med[1]:.2f} {med[2]:.2f} {med[3]:.2f}; median lam_std "
          f"{np.median(nr['lam_std']):.2f}")
    assert (nr["ndata"] == 8).all() and np.isfinite(nr["lam_mean"]).all()
    assert med[2:].min() > med[:2].max()


def test_refusals(ctx):
    nx = ny = 5
    nz, kmax = 4, 6
    sh = (ny - 2, nx - 2)
    args = dict(nx=nx, ny=ny, nz=nz, kmax=kmax, nchain=8, nbin=10, seed=1, vel0=np.full((nz, ny, nx), 3.5, np.float32),
                vmin=np.full((nz - 1,) + sh, 3.0, np.float32), vmax=np.full((nz - 1,) + sh, 4.0, np.float32),
                cobs=np.full((kmax,) + sh, 3.5, np.float32), wdat=np.ones((kmax,) + sh, np.float32), step=0.05, nadapt=50)
    mc = ctx.mc_create(**args)
    pv = np.full((kmax, mc.ncol), 3.4)
    amap, wa = np.zeros((2, kmax) + sh, np.float32), np.ones((kmax,) + sh, np.float32)

    def refused(call, word=None):
        with pytest.raises(dz.DazimError) as e:
            call()
        assert e.value.code == dz.DAZIM_E_BAD_ARG
        if word:
            assert word in str(e.value), str(e.value)

    # bad segment tables, and lengths that do not sum to kmax
    for segs in ([], [RC + (2,), RG + (2,), LC + (1,), LG + (1,), RC + (0,)], [(3, 0, kmax)], [(0, 0, kmax)], [(2, 2, kmax)], [(2, -1, kmax)],
                 [RC + (0,), RG + (kmax,)], [RC + (3,), RC + (3,)], [RC + (61,)], [RC + (3,), LG + (2,)], [RC + (4,), LG + (3,)]):
        refused(lambda: mc.set_segments(segs))
    # the groups
    g = np.arange(kmax) % 2
    refused(lambda: mc.set_noise_groups(g, [], []))                                          # ngroup 0
    refused(lambda: mc.set_noise_groups(np.arange(kmax) % 5, [2.0] * 5, [1.0] * 5))          # ngroup 5
    refused(lambda: mc.set_noise_groups(np.arange(kmax) % 3, [2.0] * 2, [1.0] * 2))          # a group index out of range
    refused(lambda: mc.set_noise_groups(-g, [2.0] * 2, [1.0] * 2))
    refused(lambda: mc.set_noise_groups(g[:-1], [2.0] * 2, [1.0] * 2))
    refused(lambda: mc.set_noise_groups(g, [2.0, 0.0], [1.0, 1.0]))                          # zero and positive a0
    for bad in (-1.0, float("inf"), float("-inf"), float("nan")):
        refused(lambda: mc.set_noise_groups(g, [2.0, bad], [1.0, 1.0]))
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        refused(lambda: mc.set_noise_groups(g, [2.0, 2.0], [1.0, bad]))
    assert mc.noise_groups_state() == dict(ngroup=0)
    refused(mc.noise_groups_result)                                                          # the mode off
    n2 = dz._ptr(np.zeros((2, 2, mc.ncol)))
    assert ctx.lib.dazim_mc_noise_groups_state(ctx._h, mc._h, None, None, None, None, None, n2, None) == dz.DAZIM_E_BAD_ARG
    other = dz.Context(0)
    i3 = dz._ptr(np.array([2, 1], np.int32))
    assert other.lib.dazim_mc_set_segments(other._h, mc._h, 2, i3, i3, i3) == dz.DAZIM_E_BAD_ARG
    assert other.lib.dazim_mc_noise_groups_state(other._h, mc._h, None, None, None, None, None, None, None) == dz.DAZIM_E_BAD_ARG
    other.close()
    # Gc/Gs with other segments than Rayleigh phase, in either order: Lsen_Gsc is Rayleigh-phase
    mc.set_segments([RC + (3,), LC + (3,)])
    refused(lambda: mc.set_aniso(2, amap, wa, 1.0, 0.1), "Rayleigh-phase")
    mc.set_aniso(0)                                                                          # (off is always allowed)
    mc.set_segments([RC + (kmax,)])
    mc.set_aniso(2, amap, wa, 1.0, 0.1)
    refused(lambda: mc.set_segments([RC + (3,), LC + (3,)]), "Rayleigh-phase")
    mc.set_segments([RC + (kmax,)])
    mc.set_aniso(0)
    mc.set_segments([RG + (3,), LC + (3,)])
    mc.set_noise_groups(g, [2.0, 2.0], [1.0, 0.5])
    refused(mc.noise_result)                                                                 # the single scale's result
    refused(mc.noise_groups_result)                                                          # before the first recorded step
    mc.step(pv, 0)
    refused(lambda: mc.set_segments([RC + (kmax,)]))                                         # the setters after a step
    refused(lambda: mc.set_noise_groups(g, [2.0, 2.0], [1.0, 1.0]))
    refused(lambda: mc.set_noise_groups(g, [0.0, 0.0], [1.0, 1.0]))
    mc.step(pv, 1)
    r = mc.noise_groups_result()                                                             # the handle still works
    assert r["lam_mean"].shape == (2,) + sh and (r["ndata"] == kmax // 2).all() and (r["lam_mean"] > 0).all() and (r["lam_std"] > 0).all()
    mc.free()
