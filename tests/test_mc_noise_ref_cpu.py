"""CPU: the restatement of the hierarchical-noise sampler (tests/mc_ref.py) alone on the linear problem whose posterior is a
multivariate t, against that posterior under the bars of tests/test_column_mc_noise_gpu.py's linear test: the bars are reachable by
the arithmetic before the device is involved."""
import numpy as np

from tests import mc_ref

NBURN, NSAMPLE, NCHAIN, NBIN, SEED = 2000, 8000, 32, 64, 77


def check_linear(pb, mean, std, rhat, lam_mean, lam_std, tag):
    """the bars of the linear Student-t test, shared with the GPU test: mean within 0.1 std, std, lam_mean and lam_std within 10 %,
    R-hat < 1.05; every figure printed first"""
    dmean = np.abs(mean - pb["mu"]) / pb["sd"]
    dstd = np.abs(std / pb["sd"] - 1)
    dl1 = np.abs(lam_mean / pb["lam_mean"] - 1)
    dl2 = np.abs(lam_std / pb["lam_std"] - 1)
    print(f"\n[measured] {tag}: |mean - mu| / std max {dmean.max():.3f}; |std / analytic - 1| max {dstd.max():.3f}; R-hat max "
          f"{rhat.max():.4f}; |lam_mean / analytic - 1| max {dl1.max():.4f}; |lam_std / analytic - 1| max {dl2.max():.4f}; "
          f"analytic E[lambda] {pb['lam_mean'].min():.2f}..{pb['lam_mean'].max():.2f}; analytic std over fixed-sigma std "
          f"{(pb['sd'] / pb['sd_fixed']).min():.2f}..{(pb['sd'] / pb['sd_fixed']).max():.2f}")
    assert dmean.max() <= 0.1
    assert dstd.max() <= 0.1
    assert rhat.max() < 1.05
    assert dl1.max() <= 0.1
    assert dl2.max() <= 0.1


def test_linear_student_t_posterior_restated():
    pb = mc_ref.linear_problem()
    ncell, kmax, nlay, K = pb["ncell"], pb["kmax"], pb["nlay"], pb["K"]
    assert (pb["sd"] / pb["sd_fixed"]).min() > 1.0           # the fixed-sigma std is too small in every cell of this problem
    cells = np.arange(ncell)
    wdat = np.full((kmax, ncell), pb["w"], np.float32)
    st, tp, ns = mc_ref.sample(lambda prop: K @ prop[:nlay].astype(np.float64), NBURN, NSAMPLE, 50, cells, NCHAIN, pb["vmin"].T,
                                     pb["vmax"].T, np.full(ncell, 3.5, np.float32), pb["cobs"].T, wdat, NBIN, SEED, (pb["a0"], pb["b0"]))
    r = mc_ref.final(st, pb["vmin"].T.copy(), pb["vmax"].T.copy(), np.full((nlay, ncell), 3.5, np.float32), cells, ncell, NCHAIN, 1,
                        NSAMPLE, NSAMPLE, NBIN)
    nr = mc_ref.result(ns, wdat, cells, ncell, NCHAIN, 1)
    assert (nr["ndata"] == kmax).all() and (ns["ncnt"] == NSAMPLE).all()
    check_linear(pb, r["mean"].T, r["std"].T, r["rhat"], nr["lam_mean"], nr["lam_std"], "restatement, mode on")
