"""CPU: the restatement of the sampler with one noise scale per group of periods (tests/mc_ref.py with tests/mc_groups_ref.py) alone:
the single-scale record and a one-group record drive it to the same bytes, and on a linear problem with two groups of unequal noise it meets the bars of
tests/test_mc_noise_ref_cpu.check_linear, per group, against quadrature over the box: the bars are reachable by the arithmetic before
the device is involved (tests/test_column_mc_groups_gpu.py runs the same problem through the library)."""
import numpy as np

from tests import mc_groups_ref as gr
from tests import mc_ref
from tests.test_mc_noise_ref_cpu import NBIN, NBURN, NCHAIN, NSAMPLE, check_linear

SEED = 77
_REF = {}


def linear_reference():
    """the linear problem and its quadrature, computed once for the CPU and the GPU test"""
    if not _REF:
        pb = gr.linear_problem()
        ref, n, move = gr.reference(pb)
        print(f"\n[measured] quadrature on {n} x {n} points over the box: the moments moved by {move:.2e} relative from half that grid")
        K, w = pb["K"], float(pb["w"])
        _REF.update(pb=pb, ref=ref, sd_fixed=np.sqrt(np.diag(np.linalg.inv(K.T @ K * w ** 2))))
    return _REF["pb"], _REF["ref"], _REF["sd_fixed"]


def check_linear_groups(pb, ref, sd_fixed, mean, std, rhat, lam_mean, lam_std, tag):
    """check_linear once per group: the group's lam_mean and lam_std, and the model's mean, std and R-hat each time"""
    for g in range(len(pb["a0"])):
        check_linear(dict(mu=ref["mu"], sd=ref["sd"], sd_fixed=sd_fixed, lam_mean=ref["lam_mean"][g], lam_std=ref["lam_std"][g]), mean, std,
                     rhat, lam_mean[g], lam_std[g], f"{tag}, group {g}")


def small_problem(rng, ncs, nchain, nlay, kmax):
    ncol = ncs * nchain
    rep = lambda x: np.repeat(x, nchain, axis=-1)
    vmin = rng.uniform(3.0, 3.2, (nlay, ncs)).astype(np.float32)
    vmax = (vmin + rng.uniform(0.5, 1.0, (nlay, ncs))).astype(np.float32)
    cobs = rng.uniform(3.2, 3.8, (kmax, ncs)).astype(np.float32)
    wdat = rng.choice([0.0, 20.0, 50.0], (kmax, ncs), p=[0.2, 0.4, 0.4]).astype(np.float32)
    wdat[0] = 50.0
    return ncol, rep, vmin, vmax, cobs, wdat


def forward_with_gaps(rng, kmax):
    """curves near 3.5 with a few periods without a root"""
    def f(prop):
        pv = 3.5 + 0.1 * rng.standard_normal((kmax, prop.shape[1]))
        pv[rng.random(pv.shape) < 0.03] = 0.0
        return pv
    return f


def test_one_group_is_mc_ref_sample_and_result():
    """sample() driven with the single-scale record against sample() driven with a one-group record, tempered and kind 1, with
    periods without data and without a root: state, ladder, record and result byte for byte"""
    for ntemp, kind in ((1, 0), (3, 1)):
        ncs, nchain, nlay, kmax = 3, 6, 3, 5
        ncol, rep, vmin, vmax, cobs, wdat = small_problem(np.random.default_rng(3), ncs, nchain, nlay, kmax)
        cells = np.array([0, 2, 5])
        args = (30, 8, 4, cells, nchain, vmin, vmax, np.full(ncs, 4.0, np.float32), cobs, wdat, 12, 99)
        kw = dict(ntemp=ntemp, tmax=8.0, nswap=2, kind=kind)
        st, tp, ns = mc_ref.sample(forward_with_gaps(np.random.default_rng(4), kmax), *args, (0.25, 0.5), **kw)
        gst, gtp, gs = mc_ref.sample(forward_with_gaps(np.random.default_rng(4), kmax), *args, (np.zeros(kmax, np.int32), [0.25], [0.5]),
                                     **kw)
        assert "ngroup" not in ns and gs["ngroup"] == 1                  # each record came back in the form it went in
        for k in st:
            assert np.asarray(st[k]).tobytes() == np.asarray(gst[k]).tobytes(), k
        for k in ("scale", "swap_try", "swap_acc"):
            assert tp[k].tobytes() == gtp[k].tobytes(), k
        assert ns["nsum"].tobytes() == gs["nsum"].tobytes() and ns["ncnt"].tobytes() == gs["ncnt"].tobytes()
        assert gs["chi2g"][0].tobytes() == gst["chi2"].tobytes()
        assert ns["ncnt"].sum() > 0
        wc = np.zeros((kmax, 6), np.float32)
        wc[:, cells] = wdat
        a, b = mc_ref.result(ns, wc, cells, 6, nchain, ntemp), gr.result(gs, wc, cells, 6, nchain, ntemp)
        for k in a:
            assert a[k].tobytes() == b[k][0].tobytes(), k


def test_groups_split_the_total():
    """two and four groups: chi2 stays the one total, each chi2_g is the group's own sum, a period without a root makes both +inf,
    and the energy leaves out a group without data"""
    rng = np.random.default_rng(8)
    kmax, ncol = 8, 40
    pv = 3.5 + 0.1 * rng.standard_normal((kmax, ncol))
    pv[2, :5] = 0.0
    cobs = rng.uniform(3.3, 3.7, (kmax, ncol)).astype(np.float32)
    wdat = np.full((kmax, ncol), 30.0, np.float32)
    wdat[1::2, 10:20] = 0.0                                    # group 1 of p % 2 without data in these columns
    for grp in (np.arange(kmax) % 2, np.arange(kmax) // 2):
        G = int(grp.max()) + 1
        tot, cg = gr.chi2_groups(pv, cobs, wdat, grp, G)
        assert tot.tobytes() == mc_ref.chi2(pv, cobs, wdat).tobytes()
        for g in range(G):
            w = np.where((grp == g)[:, None], wdat, np.float32(0))
            assert cg[g].tobytes() == mc_ref.chi2(pv, cobs, w).tobytes(), g
        assert np.isinf(tot[:5]).all() and np.isinf(cg[grp[2], :5]).all() and np.isfinite(np.delete(cg, grp[2], axis=0)[:, :5]).all()
        ndg = gr.ndata_groups(wdat, grp, G)
        x = gr.energy_groups(tot, cg, ndg, np.full(G, 2.0), np.full(G, 1.0))
        assert np.isinf(x[:5]).all() and np.isfinite(x[5:]).all()
        if G == 2:
            assert (ndg[1, 10:20] == 0).all()
            one = mc_ref.energy(cg[0, 10:20], 2.0 + 0.5 * ndg[0, 10:20], 1.0)
            assert x[10:20].tobytes() == one.tobytes()


def test_linear_two_groups_restated():
    pb, ref, sd_fixed = linear_reference()
    ncell, kmax, nlay, K = pb["ncell"], pb["kmax"], pb["nlay"], pb["K"]
    cells = np.arange(ncell)
    wdat = np.full((kmax, ncell), pb["w"], np.float32)
    st, tp, gs = mc_ref.sample(lambda prop: K @ prop[:nlay].astype(np.float64), NBURN, NSAMPLE, 50, cells, NCHAIN, pb["vmin"].T,
                               pb["vmax"].T, np.full(ncell, 3.5, np.float32), pb["cobs"].T, wdat, NBIN, SEED, (pb["grp"], pb["a0"], pb["b0"]))
    r = mc_ref.final(st, pb["vmin"].T.copy(), pb["vmax"].T.copy(), np.full((nlay, ncell), 3.5, np.float32), cells, ncell, NCHAIN, 1,
                     NSAMPLE, NSAMPLE, NBIN)
    nr = gr.result(gs, wdat, cells, ncell, NCHAIN, 1)
    assert (nr["ndata"] == kmax // 2).all() and (gs["ncnt"] == NSAMPLE).all()
    print(f"\n[measured] quadrature E[lambda_0] {ref['lam_mean'][0].min():.2f}..{ref['lam_mean'][0].max():.2f}, E[lambda_1] "
          f"{ref['lam_mean'][1].min():.2f}..{ref['lam_mean'][1].max():.2f}")
    assert np.median(ref["lam_mean"][1]) > 2 * np.median(ref["lam_mean"][0])      # the problem does separate the two levels
    check_linear_groups(pb, ref, sd_fixed, r["mean"].T, r["std"].T, r["rhat"], nr["lam_mean"], nr["lam_std"], "restatement")


def test_groups_with_prior_counts_restated():
    """the shapes of tests/test_column_mc_groups_gpu.test_groups_with_prior_step_against_numpy on host_forward's curves, by the
    restatement alone: decisions other than the energies alone would take, states with exactly one group at +inf and, with the
    ladder, every case of the swap rule do occur, so the GPU test may ask for them"""
    from tests.test_column_mc_groups_gpu import GROUPS
    from tests.test_column_mc_noise_gpu import NADAPT, NREC, SHAPES
    from tests.test_column_mc_temper_gpu import host_forward, step_problem
    for shape, G in (("untempered", 4), ("odd1", 2)):
        (nz, nchain, ntemp, nswap, kind), nburn = SHAPES[shape]
        rng, nx, ny, kmax, vel0, vmin, vmax, cobs, wdat = step_problem(nz)
        nlay = nz - 1
        cells = np.nonzero((wdat.reshape(kmax, -1) != 0).any(axis=0))[0]
        pick = lambda x: x.reshape(x.shape[0], -1)[:, cells]
        vref = (vmin + np.random.default_rng(nz).uniform(0.1, 0.9, vmin.shape) * (vmax - vmin)).astype(np.float32)
        cb = np.repeat(pick(cobs), nchain, axis=-1)
        n = dict(dec=0, swap=0, ninf_group=0, seen=dict.fromkeys(mc_ref.BRANCHES, 0), t=0)

        def each(t, r):
            n["dec"] += r["diff"]["dec"]
            n["swap"] += r["diff"]["swap"]
            n["ninf_group"] += int((np.isinf(r["ns"]["chi2g"]).sum(axis=0) == 1).sum())
            for k in r["seen"]:
                n["seen"][k] += r["seen"][k]

        def forward(prop):
            n["t"] += 1
            return host_forward(rng, cb, n["t"], nswap)
        mc_ref.sample(forward, nburn, NREC, NADAPT, cells, nchain, pick(vmin), pick(vmax), pick(vel0[nlay:, 1:-1, 1:-1])[0], pick(cobs),
                      pick(wdat), 20, 0x1234_5678_9ABC, GROUPS[G], (3.0, 4.0, pick(vref)), ntemp=ntemp, tmax=16.0, nswap=nswap, kind=kind,
                      each=each)
        print(f"\n[measured] {shape}, {G} groups and the prior, restated: {n}")
        assert n["dec"] > 0 and n["ninf_group"] > 0
        if ntemp > 1:
            assert all(v > 0 for v in n["seen"].values()), n["seen"]
