"""-m gpu: radial anisotropy in the Monte-Carlo sampler (dazim_mc_set_radial).

Every step of a radial handle bit for bit against the NumPy restatement (tests/mc_ref.py's step through tests/mc_step_check.drive
with tests/mc_radial_ref.py's Q in place, plus the radial record and the Vsv model after every step), the final statistics, every
refusal, dazim_mc_run against the hand loop of its own parts, the linear-Gaussian problem under the bars that the restatement set
(tests/test_mc_radial_ref_cpu.py), and the dispersion forward model on an isotropic and on a radially anisotropic truth."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_radial_ref as rr
from tests import mc_ref, mc_step_check
from tests.bars import within
from tests.mc_step_check import check_final, drive, ulps
from tests.test_column_mc_gpu import create, per_column
from tests.test_column_mc_temper_gpu import host_forward

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    dz.build()
    c = dz.Context(0)
    yield c
    c.close()


NADAPT, NREC = 4, 8
SMOOTH, DAMP, COUPLE = 3.0, 4.0, 5.0
# n, (nx, ny), nchain, ntemp, (kR, kL), kind, noise groups, prior, couple, burn-in.  Kind 1 reaches its first factor inside the burn-in:
# 8 * 2n states over the chains are 12 decisions at "b" (7 chains), 8 at "d" (64 chains) and 6 at "e" (6 chains)
SHAPES = {
    "a": (1, (4, 3), 1, 1, (2, 1), 0, False, True, COUPLE, 12),           # n = 1, 2 cells, 1 chain
    "b": (5, (4, 4), 7, 1, (3, 2), 1, False, True, COUPLE, 13),           # a Philox block of four knots straddles the boundary
    "c": (3, (5, 3), 8, 4, (3, 3), 0, True, True, COUPLE, 12),            # Rayleigh only, Love only and no data; one group per type
    "d": (31, (3, 3), 64, 1, (2, 2), 1, False, True, COUPLE, 12),         # the LDS and lane bound
    "e": (2, (4, 4), 6, 1, (2, 2), 1, False, False, 0.0, 12),             # couple 0, prior off
}


def problem(shape):
    n, (nx, ny), nchain, ntemp, (kr, kl), kind, groups, prior, couple, nburn = SHAPES[shape]
    rng = np.random.default_rng(17 + n)
    nz, kmax = 2 * n + 1, kr + kl
    sh = (ny - 2, nx - 2)
    vel0 = rng.uniform(3.0, 4.5, (nz, ny, nx)).astype(np.float32)
    vmin = rng.uniform(2.8, 3.4, (2 * n,) + sh).astype(np.float32)
    vmax = (vmin + rng.uniform(0.3, 1.2, vmin.shape)).astype(np.float32)
    cobs = rng.uniform(3.2, 4.0, (kmax,) + sh).astype(np.float32)
    wdat = rng.uniform(50, 150, (kmax,) + sh).astype(np.float32)
    if shape == "c":
        wdat[kr:, 0, 0] = 0.0          # Rayleigh data only
        wdat[:kr, 0, 1] = 0.0          # Love data only
        wdat[:, 0, 2] = 0.0            # no data
    segments = [(2, 0, np.linspace(6.0, 30.0, kr)), (1, 0, np.linspace(7.0, 35.0, kl))]
    return rng, nx, ny, nz, kmax, vel0, vmin, vmax, cobs, wdat, segments


def radial_handle(ctx, shape, radial=True, nbin=20, seed=0x1234_5678_9ABC):
    n, _, nchain, ntemp, (kr, kl), kind, groups, prior, couple, nburn = SHAPES[shape]
    rng, nx, ny, nz, kmax, vel0, vmin, vmax, cobs, wdat, segments = problem(shape)
    mc = create(ctx, nx, ny, nz, kmax, nchain, nbin, seed, vel0, vmin, vmax, cobs, wdat, 0.05, NADAPT)
    mc.set_segments(segments)
    vref = (vmin + np.random.default_rng(n).uniform(0.1, 0.9, vmin.shape) * (vmax - vmin)).astype(np.float32)
    if prior and shape in ("a", "c"):               # the two setters in either order
        mc.set_prior(SMOOTH, DAMP, vref)
    if kind == 1:
        mc.set_proposal(1)
    if ntemp > 1:
        mc.set_tempering(ntemp, 16.0, 1)
    if groups:
        mc.set_noise_groups([0] * kr + [1] * kl, [0.25, 0.5], [0.5, 0.25])
    if radial:
        mc.set_radial(couple)
    if prior and shape not in ("a", "c"):
        mc.set_prior(SMOOTH, DAMP, vref)
    return mc, rng, vel0, vmin, vmax, cobs, wdat, vref, segments


@pytest.mark.parametrize("shape", ["a", "b", "c", "d"])
def test_radial_step_against_numpy(ctx, shape, monkeypatch):
    """burn-in steps (adaptation every 4) and 8 recorded ones on hand-made curves, every step restated from the library's own
    state: what tests/mc_step_check.drive compares, with the radial Q where drive and mc_ref.step look Q up; after every step the
    radial record bit for bit against the restated record of the new states, and the Vsv and Vsh models against the split of the new
    proposals.  Then radial_result against the restated final statistics: counts, means and quantiles exact, what passes through a
    square root within one fp32 ulp."""
    n, _, nchain, ntemp, (kr, kl), kind, groups, prior, couple, nburn = SHAPES[shape]
    nbin, seed = 20, 0x1234_5678_9ABC
    mc, rng, vel0, vmin, vmax, cobs, wdat, vref, _ = radial_handle(ctx, shape, nbin=nbin, seed=seed)
    q = rr.prior_q_of(couple)
    monkeypatch.setattr(mc_ref, "prior_q", q)
    monkeypatch.setattr(mc_step_check, "prior_q", q)
    nlay = 2 * n
    assert mc.nlay == nlay and mc.radial_state()["n"] == n and mc.radial_state()["couple"] == couple
    lo, hi = per_column(vmin.astype(np.float64), mc), per_column(vmax.astype(np.float64), mc)
    cb, wd, vr = per_column(cobs, mc), per_column(wdat, mc), per_column(vref, mc)
    ps = mc.prior_state()
    assert (ps["smooth"], ps["damp"]) == (SMOOTH, DAMP) and np.array_equal(ps["vref"], vref)
    assert np.array_equal(ps["q"], q(mc.state()["cur"][:nlay], vr, SMOOTH, DAMP))     # the start models, in either order of the setters
    _, cs, rung, _ = mc_ref.layout(mc.ncol, nchain, ntemp, mc._cells)
    box = dict(rs=rr.empty_record(n, mc.ncol, mc.ncs, nbin, couple), checked=0)

    def check_radial(t_done):
        """after step t_done: the record and the two models"""
        cur = mc.state()["cur"]
        if t_done > nburn:
            box["rs"] = rr.record(box["rs"], cur, rung == 0, cs, lo, hi, nbin)
        got = mc.radial_state()
        for k in ("rsum", "ngt1", "xhist"):
            assert np.array_equal(got[k], box["rs"][k]), (t_done, k)
        vsv, vsh = (m.cpu().numpy() for m in mc.radial_models())
        evsv, evsh = rr.split(mc.proposals().cpu().numpy())
        assert np.array_equal(vsv, evsv) and np.array_equal(vsh, evsh), t_done
        box["checked"] += 1

    def forward(t):
        check_radial(t - 1)                      # (t = 1: the start models, nothing recorded)
        return host_forward(rng, cb, t, 1)

    run = drive(mc, forward, nburn, NREC, NADAPT, lo, hi, cb, wd, nbin, seed, vref=vr)
    check_radial(nburn + NREC)
    assert box["checked"] == nburn + NREC + 1
    got, gtp, gcov, rs = run["got"], run["gtp"], run["gcov"], box["rs"]
    print(f"\n[measured] {shape}: decisions {run['ndec']} accepted, {run['ndiff_dec']} other than the energies alone; swaps "
          f"{int(gtp['swap_acc'].sum())} of {int(gtp['swap_try'].sum())}; factors {run['nfact']}; xi > 1 in {int(rs['ngt1'].sum())} of "
          f"{int(rs['xhist'].sum())} recorded (state, pair)s")
    assert run["ndec"] > 0 and (run["ndiff_dec"] > 0 or shape == "a")       # ("a": 2 chains take 38 decisions)
    assert rs["xhist"].sum() == mc.ncs * (nchain // ntemp) * n * NREC and 0 < rs["ngt1"].sum() < rs["xhist"].sum()
    if kind == 1:
        assert (gcov["cov_set"] == 1).all() and run["nfact"] >= mc.ncs
    if groups:
        assert run["gns"]["ncnt"].sum() > 0
    check_final(mc, got, vmin, vmax, vel0, ntemp, NREC, nbin)
    ncell = mc.ncell
    e = rr.final(got, rs, vmin.reshape(nlay, ncell), vmax.reshape(nlay, ncell), vel0[:nlay, 1:-1, 1:-1].reshape(nlay, ncell), mc._cells,
                 ncell, nchain, ntemp, NREC, nbin)
    r = mc.radial_result()
    for k in ("xi_mean", "xi_q", "p_gt1", "voigt_mean"):
        assert np.array_equal(r[k].reshape(e[k].shape), e[k], equal_nan=True), k
    for k in ("xi_std", "xi_rhat", "corr_vh", "voigt_std"):
        a, b = r[k].reshape(e[k].shape), e[k]
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), k
        if fin.any():
            assert ulps(a[fin], b[fin]).max() <= 1, k
    if shape == "c":                              # the cell without data: the start model, NaN where nothing was sampled
        assert mc.n_empty == 1 and np.isnan(r["p_gt1"][:, 0, 2]).all() and (r["xi_std"][:, 0, 2] == 0).all()
        assert np.isfinite(r["p_gt1"][:, 0, :2]).all()
    # each output is nullable
    one = np.zeros((n, mc.ny - 2, mc.nx - 2), np.float32)
    ctx._check(ctx.lib.dazim_mc_radial_result(ctx._h, mc._h, None, None, None, None, dz._ptr(one), None, None, None))
    assert np.array_equal(one, r["p_gt1"], equal_nan=True)
    mc.free()


def test_no_coupling_no_prior_is_the_stacked_handle(ctx):
    """shape (e): set_radial(0) without a prior leaves every field of state, cov_state and the Vs result equal to the same handle
    without set_radial, over 12 + 8 steps of kind 1 on the same hand-made curves"""
    out = {}
    for radial in (False, True):
        mc, rng, vel0, vmin, vmax, cobs, wdat, _, _ = radial_handle(ctx, "e", radial=radial)
        cb = per_column(cobs, mc)
        assert mc.prior_state() == dict(smooth=0.0, damp=0.0)
        for t in range(1, 21):
            mc.step(host_forward(rng, cb, t, 1), int(t > 12))
        out[radial] = {"state." + k: v for k, v in mc.state().items() if k != "step"}
        out[radial].update({"cov." + k: v for k, v in mc.cov_state().items() if k != "kind"})
        out[radial].update({"result." + k: v for k, v in mc.result().items()})
        out[radial]["prop"] = mc.proposals().cpu().numpy()
        if radial:
            assert mc.radial_state()["xhist"].sum() == mc.ncs * mc.nchain * 2 * 8
        mc.free()
    assert out[False].keys() == out[True].keys() and out[True]["cov.cov_set"].all()
    for k in out[False]:
        assert out[False][k].tobytes() == out[True][k].tobytes(), k


def test_refusals(ctx):
    n, nx, ny, kr, kl = 2, 5, 5, 3, 2
    nz, kmax = 2 * n + 1, kr + kl
    sh = (ny - 2, nx - 2)
    args = dict(nx=nx, ny=ny, nz=nz, kmax=kmax, nchain=8, nbin=10, seed=1, vel0=np.full((nz, ny, nx), 3.5, np.float32),
                vmin=np.full((nz - 1,) + sh, 3.0, np.float32), vmax=np.full((nz - 1,) + sh, 4.0, np.float32),
                cobs=np.full((kmax,) + sh, 3.5, np.float32), wdat=np.ones((kmax,) + sh, np.float32), step=0.05, nadapt=50)
    tr, tl = np.linspace(6.0, 20.0, kr), np.linspace(8.0, 24.0, kl)
    good = [(2, 0, tr), (1, 0, tl)]

    def refused(call):
        with pytest.raises(dz.DazimError) as e:
            call()
        assert e.value.code == dz.DAZIM_E_BAD_ARG

    mc = ctx.mc_create(**args)
    refused(lambda: mc.set_radial(5.0))                                    # no segments: Rayleigh phase alone
    assert ctx.lib.dazim_mc_radial_models(mc._h, None, None, None) == dz.DAZIM_E_BAD_ARG
    assert mc.radial_state() == dict(n=0, couple=0.0)
    d = dz._ptr(np.zeros((5, n, mc.ncol)))
    assert ctx.lib.dazim_mc_radial_state(ctx._h, mc._h, None, None, d, None, None) == dz.DAZIM_E_BAD_ARG
    refused(mc.radial_result)
    for bad in ([(1, 0, tl), (2, 0, tr)],                                  # Love before Rayleigh
                [(2, 0, tr), (2, 1, tl)],                                  # no Love segment
                [(1, 0, tr), (1, 1, tl)],                                  # no Rayleigh segment
                [(2, 0, tr[:2]), (1, 0, tl), (2, 1, tr[2:])]):             # a Rayleigh segment behind a Love segment
        mc.set_segments(bad)
        refused(lambda: mc.set_radial(5.0))
    mc.set_segments(good)
    for bad in (-1.0, -1e-30, float("inf"), float("-inf"), float("nan")):
        refused(lambda: mc.set_radial(bad))
    other = dz.Context(0)
    assert other.lib.dazim_mc_set_radial(other._h, mc._h, 5.0) == dz.DAZIM_E_BAD_ARG
    assert other.lib.dazim_mc_radial_result(other._h, mc._h, *([None] * 8)) == dz.DAZIM_E_BAD_ARG
    other.close()
    mc.set_radial(5.0)
    mc.set_radial(0.0)                                                     # a second call replaces the coupling
    assert mc.radial_state()["couple"] == 0.0 and mc.prior_state() == dict(smooth=0.0, damp=0.0)
    mc.set_radial(5.0)
    assert "q" in mc.prior_state()                                         # the coupling alone puts the prior on
    refused(lambda: mc.set_aniso(2, np.zeros((2, kmax) + sh, np.float32), np.ones((kmax,) + sh, np.float32), 1.0, 1.0))
    refused(lambda: mc.set_segments([(1, 0, tl), (2, 0, tr)]))             # a radial handle keeps Rayleigh before Love
    mc.set_segments([(2, 0, tr[:2]), (2, 1, tr[2:]), (1, 0, tl)])          # another split that keeps the order
    mc.set_segments(good)
    refused(mc.radial_result)                                              # no recorded step yet
    pv = np.full((kmax, mc.ncol), 3.4)
    mc.step(pv, 0)
    refused(lambda: mc.set_radial(5.0))                                    # after a step
    refused(lambda: mc.set_radial(0.0))
    mc.step(pv, 1)
    r = mc.radial_result()
    assert np.isfinite(r["xi_mean"]).all() and np.isfinite(r["voigt_mean"]).all()
    mc.free()
    # nz - 1 odd
    odd = dict(args, nz=nz + 1, vel0=np.full((nz + 1, ny, nx), 3.5, np.float32), vmin=np.full((nz,) + sh, 3.0, np.float32),
               vmax=np.full((nz,) + sh, 4.0, np.float32))
    mc = ctx.mc_create(**odd, segments=good)
    refused(lambda: mc.set_radial(5.0))
    mc.free()
    # a vmin <= 0
    for v in (0.0, -1.0):
        low = dict(args, vmin=args["vmin"].copy())
        low["vmin"][3, 1, 2] = v
        mc = ctx.mc_create(**low, segments=good)
        refused(lambda: mc.set_radial(5.0))
        mc.free()
    # Gc/Gs and radial: whichever comes second fails
    mc = ctx.mc_create(**args)
    mc.set_aniso(2, np.zeros((2, kmax) + sh, np.float32), np.ones((kmax,) + sh, np.float32), 1.0, 1.0)
    refused(lambda: mc.set_radial(5.0))
    mc.free()
    refused(lambda: ctx.mc_create(**args, radial=5.0))                     # through mc_create: no segments
    mc = ctx.mc_create(**args, segments=good, radial=5.0)
    assert mc.radial_state()["n"] == n
    mc.free()


def disp_problem(ctx, nx, ny, depz, tr, tl, truth_v, truth_h, sigma):
    """exact Rayleigh curves of truth_v and Love curves of truth_h [n+1][ny][nx] at the inner cells -> cobs, wdat [kR+kL][ny-2][nx-2]"""
    pr, _, nf = ctx.dispersion_kernels_typed(truth_v, depz, [(2, 0, tr)], 3.0, kernels=False)
    pl, _, nl = ctx.dispersion_kernels_typed(truth_h, depz, [(1, 0, tl)], 3.0, kernels=False)
    assert nf == 0 and nl == 0
    cobs = np.concatenate([pr.reshape(len(tr), ny, nx), pl.reshape(len(tl), ny, nx)])[:, 1:-1, 1:-1].astype(np.float32)
    return cobs, np.full(cobs.shape, 1.0 / sigma, np.float32)


def stacked(v, h):
    """[Vsv knots, Vsh knots, the deepest knot] from two profiles [n+1][..]"""
    return np.concatenate([v[:-1], h[:-1], v[-1:]])


def test_run_against_hand_loop(ctx):
    """dazim_mc_run equals the hand loop radial_models() -> two dispersion_kernels_typed(kernels=False) -> step(), byte for byte in
    state, radial state and both results, with proposal 1, tempering, one noise group per wave type and the prior all on; the run's
    stats name the mode"""
    nx = ny = 5
    depz = np.array([0.0, 8.0, 20.0, 35.0], np.float32)
    tr, tl = np.array([6.0, 10.0, 16.0, 24.0, 32.0]), np.array([7.0, 12.0, 20.0, 30.0])
    n, kr, kl = len(depz) - 1, len(tr), len(tl)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    tv = np.stack([2.9 + 0.03 * z + 0.1 * np.sin(0.9 * ii + 0.5 * k) * np.cos(0.7 * jj) for k, z in enumerate(depz)]).astype(np.float32)
    th = (tv * np.float32(1.03)).astype(np.float32)
    th[-1] = tv[-1]
    cobs, wdat = disp_problem(ctx, nx, ny, depz, tr, tl, tv, th, 0.01)
    vel0 = stacked(tv, tv)
    vmin, vmax = vel0[:-1, 1:-1, 1:-1] - np.float32(0.4), vel0[:-1, 1:-1, 1:-1] + np.float32(0.4)
    segs = [(2, 0, tr), (1, 0, tl)]
    nburn, nrec = 25, 10
    out = {}
    for how in ("run", "loop"):
        mc = ctx.mc_create(nx, ny, 2 * n + 1, kr + kl, 8, 40, 3, vel0, vmin, vmax, cobs, wdat, nadapt=5, proposal=1, ntemp=2, tmax=8.0,
                           segments=segs, noise_groups=([0] * kr + [1] * kl, [2.0, 2.0], [1.0, 1.0]), prior=(2.0, 1.0), radial=5.0)
        if how == "run":
            mc.run(depz, 3.0, np.concatenate([tr, tl]), nburn, nrec)
            assert ctx.stat("mc.radial") == 1 and ctx.stat("mc.prior") == 1 and ctx.stat("mc.disp") > 0 and ctx.stat("mc.steps") == nburn + nrec
        else:
            for t in range(nburn + nrec):
                vsv, vsh = mc.radial_models()
                pr, _, _ = ctx.dispersion_kernels_typed(vsv.reshape(n + 1, 1, -1), depz, segs[:1], 3.0, kernels=False)
                pl, _, _ = ctx.dispersion_kernels_typed(vsh.reshape(n + 1, 1, -1), depz, segs[1:], 3.0, kernels=False)
                import torch
                mc.step(torch.cat([pr, pl]), int(t >= nburn))
        o = {"state." + k: v for k, v in mc.state().items() if k != "step"}
        for name, d in (("radial.", mc.radial_state()), ("result.", mc.result()), ("rresult.", mc.radial_result()),
                        ("cov.", mc.cov_state()), ("temper.", mc.temper_state()), ("noise.", mc.noise_groups_state()),
                        ("prior.", mc.prior_state())):
            o.update({name + k: v for k, v in d.items() if isinstance(v, np.ndarray)})
        out[how] = o
        mc.free()
    assert out["run"].keys() == out["loop"].keys() and "radial.xhist" in out["run"] and "rresult.xi_q" in out["run"]
    for k in out["run"]:
        assert out["run"][k].tobytes() == out["loop"][k].tobytes(), k
    assert out["run"]["radial.xhist"].sum() == 9 * 4 * n * nrec and np.isfinite(out["run"]["state.chi2"]).all()


def test_linear_gaussian_posterior(ctx):
    """tests/mc_radial_ref.linear_problem on the device (32 chains, kind 0, 1500 + 4000 steps, the seed of the restatement's run)
    under LINEAR_BARS, twice the restatement's own figures (tests/test_mc_radial_ref_cpu.py).  Measured on an MI355X: the
    restatement's figures to every printed digit (0.0308 sd, 0.0168, 0.0217, 0.0261 sd, 0.0155, 0.0063; R-hat 1.0037, of xi 1.0027)"""
    import torch
    pb = rr.linear_problem()
    n, ncell, nchain, nbin = pb["n"], pb["ncell"], 32, 64
    nx = ny = 6
    sh = (ny - 2, nx - 2)
    kmax = pb["kr"] + pb["kl"]
    vel0 = np.full((2 * n + 1, ny, nx), 3.5, np.float32)
    mc = ctx.mc_create(nx, ny, 2 * n + 1, kmax, nchain, nbin, 77, vel0, pb["vmin"].T.reshape((2 * n,) + sh), pb["vmax"].T.reshape((2 * n,) + sh),
                       pb["cobs"].T.reshape((kmax,) + sh), np.full((kmax,) + sh, pb["w"], np.float32), nadapt=50,
                       segments=[(2, 0, np.arange(pb["kr"]) + 5.0), (1, 0, np.arange(pb["kl"]) + 5.0)], prior=(pb["smooth"], pb["damp"]),
                       radial=pb["couple"])
    dev = torch.device("cuda", ctx.device)
    KR, KL = torch.tensor(pb["KR"], device=dev), torch.tensor(pb["KL"], device=dev)
    nburn, nsample = rr.LINEAR_STEPS
    for t in range(nburn + nsample):
        vsv, vsh = mc.radial_models()
        mc.step(torch.cat([KR @ vsv[:n].double(), KL @ vsh[:n].double()]), int(t >= nburn))
    r, f = mc.result(), mc.radial_result()
    flat = lambda a: a.reshape(a.shape[0], ncell).T
    fig = rr.linear_figures(pb, flat(r["mean"]), flat(r["std"]), flat(f["corr_vh"]), flat(f["xi_mean"]), flat(f["xi_std"]), flat(f["p_gt1"]))
    print(f"\n[measured] R-hat max {r['rhat'].max():.4f}, of xi {f['xi_rhat'].max():.4f}; acceptance {r['accept'].min():.3f}.."
          f"{r['accept'].max():.3f}")
    for k, v in fig.items():
        within(f"the chains against the analytic posterior, {k}", v, rr.LINEAR_BARS[k])
    assert r["rhat"].max() < 1.05 and f["xi_rhat"].max() < 1.05
    mc.free()


def test_dispersion_forward_isotropic_and_anisotropic(ctx):
    """6 x 6 cells, n = 3 sampled knots per profile, 8 + 8 phase periods over 5 - 40 s, sigma_c 0.01, 16 chains, proposal 1,
    sigma_hv 0.2, 250 + 400 steps, one seed.  Exact curves of an isotropic truth: xi = 1 lies inside [p2.5, p97.5] at every cell and
    knot.  Vsh = 1.04 Vsv at knot 1: the true xi lies inside it everywhere, and p_gt1 at that knot exceeds the isotropic run's in
    every cell.
    Measured on an MI355X: inside at 108 of 108 (cell, knot)s in both runs, the interval's median width 0.139 and 0.143; median p_gt1
    per knot 0.54, 0.46, 0.53 (isotropic) and 0.60, 0.976, 0.58; R-hat of xi median / max 1.056 / 1.107 and 1.053 / 1.124; the median
    Vsv-Vsh correlation 0.08; no proposal without a root; 5.9 s per run, 5.8 s of it in the 1 300 dispersion calls."""
    nx = ny = 8
    depz = np.array([0.0, 10.0, 25.0, 45.0], np.float32)
    tr = tl = np.array([5.0, 8.0, 12.0, 16.0, 22.0, 28.0, 34.0, 40.0])
    n = len(depz) - 1
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    tv = np.stack([2.9 + 0.03 * z + 0.08 * np.sin(0.9 * ii + 0.5 * k) * np.cos(0.7 * jj) for k, z in enumerate(depz)]).astype(np.float32)
    ref = np.broadcast_to((2.9 + 0.03 * depz)[:, None, None], tv.shape).astype(np.float32)
    tv[-1] = ref[-1]                              # the deepest knot is not sampled: the truth's is the start model's
    vel0 = stacked(ref, ref)
    vmin, vmax = vel0[:-1, 1:-1, 1:-1] - np.float32(0.5), vel0[:-1, 1:-1, 1:-1] + np.float32(0.5)
    res = {}
    for name, fac in (("iso", 1.0), ("aniso", 1.04)):
        th = tv.copy()
        th[1] = (tv[1] * np.float32(fac)).astype(np.float32)
        cobs, wdat = disp_problem(ctx, nx, ny, depz, tr, tl, tv, th, 0.01)
        mc = ctx.mc_create(nx, ny, 2 * n + 1, 16, 16, 100, 1, vel0, vmin, vmax, cobs, wdat, proposal=1, segments=[(2, 0, tr), (1, 0, tl)],
                           radial=1.0 / 0.2)
        nr = mc.run(depz, 3.0, np.concatenate([tr, tl]), 250, 400)
        r, f = mc.result(), mc.radial_result()
        xi = (th[:n, 1:-1, 1:-1].astype(np.float64) / tv[:n, 1:-1, 1:-1]) ** 2
        inside = (f["xi_q"][0] <= xi) & (xi <= f["xi_q"][2])
        res[name] = (f, inside, xi)
        print(f"\n[measured] {name}: true xi inside [p2.5, p97.5] at {inside.sum()} of {inside.size} (cell, knot)s; interval width median "
              f"{np.median(f['xi_q'][2] - f['xi_q'][0]):.3f}; R-hat of xi median / max {np.median(f['xi_rhat']):.3f} / {f['xi_rhat'].max():.3f}; "
              f"p_gt1 per knot (median) {np.median(f['p_gt1'], axis=(1, 2))}; corr_vh median {np.median(f['corr_vh']):.3f}; proposals "
              f"without a root {nr}; mc.step {ctx.stat('mc.step'):.3f} s, mc.disp {ctx.stat('mc.disp'):.3f} s of {ctx.stat('mc'):.2f} s")
        mc.free()
    assert res["iso"][1].all(), np.argwhere(~res["iso"][1])
    assert res["aniso"][1].all(), np.argwhere(~res["aniso"][1])
    assert (res["aniso"][0]["p_gt1"][1] > res["iso"][0]["p_gt1"][1]).all()
