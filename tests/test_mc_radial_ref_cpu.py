"""The NumPy restatement of the radial Monte-Carlo mode (tests/mc_radial_ref.py) against independent arithmetic, no GPU: the radial Q
against the dense precision of dazim_column_resolution_radial, the final statistics against numpy on hand-made states, and the
restatement's own sampler against the analytic posterior of a linear-Gaussian problem, which sets the bars of the device test
(tests/test_column_mc_radial_gpu.py)."""
import numpy as np
import pytest

from tests import mc_radial_ref as rr
from tests.bars import within


@pytest.mark.parametrize("n", [1, 2, 5])
def test_q_is_the_dense_quadratic_form(n):
    """Q = [dv; dh]^T P2 [dv; dh] with P2 built densely where both profiles share their reference (the coupling acts on the model,
    the rest about vref), and [dv; dh]^T Pb [dv; dh] + mu^2 |vh - vv|^2 where they do not; to fp64 rounding of sums of 6 n positive
    terms, 1e-13 relative"""
    rng = np.random.default_rng(n)
    ncol, smooth, damp, couple = 40, 3.0, 1.5, 5.0
    v = rng.uniform(3.0, 4.0, (2 * n, ncol)).astype(np.float32)
    half = rng.uniform(3.2, 3.8, (n, ncol)).astype(np.float32)
    P2, Pb = rr.precision(n, smooth, damp, couple), rr.precision(n, smooth, damp, 0.0)
    shared = np.concatenate([half, half])
    d = v.astype(np.float64) - shared
    q, ref = rr.radial_q(v, shared, smooth, damp, couple), np.einsum("ac,ab,bc->c", d, P2, d)
    within(f"n = {n}: Q against d^T P2 d, shared reference, relative", (np.abs(q - ref) / ref).max(), 1e-13)
    other = rng.uniform(3.2, 3.8, (2 * n, ncol)).astype(np.float32)
    d = v.astype(np.float64) - other
    c = v[n:].astype(np.float64) - v[:n]
    q, ref = rr.radial_q(v, other, smooth, damp, couple), np.einsum("ac,ab,bc->c", d, Pb, d) + couple ** 2 * (c * c).sum(axis=0)
    within(f"n = {n}: Q against d^T Pb d + mu^2 |vh - vv|^2, relative", (np.abs(q - ref) / ref).max(), 1e-13)
    # each part alone, and nothing of the other parts in it
    assert np.allclose(rr.radial_q(v, other, 0.0, 0.0, couple), couple ** 2 * (c * c).sum(axis=0), rtol=1e-14, atol=0)
    assert (rr.radial_q(v, other, 0.0, 0.0, 0.0) == 0).all()


def test_split():
    prop = np.arange(7 * 3, dtype=np.float32).reshape(7, 3)
    vsv, vsh = rr.split(prop)
    assert np.array_equal(vsv, prop[[0, 1, 2, 6]]) and np.array_equal(vsh, prop[[3, 4, 5, 6]])


def hand_made():
    """2 sampled cells of 3 (the middle one without data), n = 2, 4 chains, 2 rungs (so 2 recorded chains per cell), 6 recorded
    states per chain.  Cell 0, pair 0 visits the two corners of its box where xi is the range's ends; cell 2, pair 1 never moves
    (std 0).  Returns what final() takes and the states [step][2n][cold columns]."""
    rng = np.random.default_rng(3)
    n, nchain, ntemp, nbin, nrec, ncell = 2, 4, 2, 10, 6, 3
    cells = np.array([0, 2])
    ncol = len(cells) * nchain
    vmin = rng.uniform(3.0, 3.2, (2 * n, ncell)).astype(np.float32)
    vmax = (vmin + rng.uniform(0.4, 0.8, vmin.shape)).astype(np.float32)
    vel0 = (0.5 * (vmin.astype(np.float64) + vmax)).astype(np.float32)
    rep = lambda x: np.repeat(x[:, cells], nchain, axis=1)
    lo, hi = rep(vmin.astype(np.float64)), rep(vmax.astype(np.float64))
    _, cs, rung, _ = rr.mc_ref.layout(ncol, nchain, ntemp, cells)
    cold = rung == 0
    st = dict(sums=np.zeros((2, 2 * n, ncol)))
    rs = rr.empty_record(n, ncol, len(cells), nbin)
    states = []
    for t in range(nrec):
        cur = np.concatenate([(lo + rng.random(lo.shape) * (hi - lo)).astype(np.float32), np.zeros((1, ncol), np.float32)])
        if t == 1:    # the corner of lowest xi: vv at its top, vh at its bottom; t == 2: the other corner
            cur[0, 0], cur[n, 0] = vmax[0, 0], vmin[n, 0]
        if t == 2:
            cur[0, 0], cur[n, 0] = vmin[0, 0], vmax[n, 0]
        cur[1, 4:], cur[n + 1, 4:] = np.float32(3.5), np.float32(3.625)      # cell 2, pair 1 stands still
        v = cur[:2 * n, cold].astype(np.float64)
        st["sums"][0][:, cold] += v
        st["sums"][1][:, cold] += v * v
        rs = rr.record(rs, cur, cold, cs, lo, hi, nbin)
        states.append(v)
    return dict(st=st, rs=rs, vmin=vmin, vmax=vmax, vel0=vel0, cells=cells, ncell=ncell, nchain=nchain, ntemp=ntemp, nrec=nrec,
                nbin=nbin, n=n, cold=cold, states=np.array(states))


def test_final_statistics_against_numpy():
    """final() on hand-made states against numpy's own mean, std, corrcoef and quantiles of the same states: the fp64 statistics to
    1e-6 relative (fp32 results of fp64 sums), the quantiles within one bin of numpy's; the end bins where xi sits on the range's
    ends; a pair that never moves has std 0 and no R-hat or correlation; the cell without data returns the start model"""
    h = hand_made()
    n, nbin = h["n"], h["nbin"]
    f = rr.final(h["st"], h["rs"], h["vmin"], h["vmax"], h["vel0"], h["cells"], h["ncell"], h["nchain"], h["ntemp"], h["nrec"], nbin)
    xlo, xhi = rr.xi_range(h["vmin"].astype(np.float64), h["vmax"].astype(np.float64))
    # the corners fell into the end bins, exactly on the range's ends
    assert h["rs"]["xhist"][0, 0, 0] >= 1 and h["rs"]["xhist"][0, 0, nbin - 1] >= 1
    assert h["rs"]["xhist"].sum() == 2 * 2 * n * h["nrec"] and h["rs"]["ngt1"].sum() > 0
    ncold = h["nchain"] // h["ntemp"]
    for ci, cell in enumerate(h["cells"]):
        v = h["states"][:, :, ci * ncold:(ci + 1) * ncold]              # [step][2n][cold chain]
        for a in range(n):
            vv, vh = v[:, a].ravel(), v[:, n + a].ravel()
            xi = (vh / vv) ** 2
            V = np.sqrt((2 * vv ** 2 + vh ** 2) / 3)
            still = cell == 2 and a == 1
            rel = lambda got, ref: abs(float(got) - ref) / max(abs(ref), 1e-30)
            assert rel(f["xi_mean"][a, cell], xi.mean()) <= 1e-6 and rel(f["voigt_mean"][a, cell], V.mean()) <= 1e-6
            assert f["p_gt1"][a, cell] == np.float32((xi > 1).mean())
            if still:
                assert f["xi_std"][a, cell] <= 1e-7 and f["voigt_std"][a, cell] <= 1e-6
                assert np.isnan(f["corr_vh"][a, cell]) and (np.isnan(f["xi_rhat"][a, cell]) or f["xi_std"][a, cell] > 0)
                assert f["p_gt1"][a, cell] == 1.0
            else:
                assert rel(f["xi_std"][a, cell], xi.std()) <= 1e-5 and rel(f["voigt_std"][a, cell], V.std()) <= 1e-4
                assert abs(f["corr_vh"][a, cell] - np.corrcoef(vv, vh)[0, 1]) <= 1e-5
                # R-hat from the chains' own means and variances
                x = ((v[:, n + a] / v[:, a]) ** 2)                      # [step][chain]
                N = x.shape[0]
                W, B = x.var(axis=0, ddof=1).mean(), N * x.mean(axis=0).var(ddof=1)
                assert rel(f["xi_rhat"][a, cell], np.sqrt(((N - 1) / N * W + B / N) / W)) <= 1e-5
            width = (xhi[a, cell] - xlo[a, cell]) / nbin
            for e, qv in enumerate((0.025, 0.5, 0.975)):
                assert abs(f["xi_q"][e, a, cell] - np.quantile(xi, qv)) <= width + 1e-6, (cell, a, e)
    # the cell without data
    v0 = h["vel0"].astype(np.float64)[:, 1]
    for a in range(n):
        xi0 = np.float32((v0[n + a] / v0[a]) ** 2)
        assert f["xi_mean"][a, 1] == xi0 and (f["xi_q"][:, a, 1] == xi0).all() and f["xi_std"][a, 1] == 0 and f["voigt_std"][a, 1] == 0
        assert f["voigt_mean"][a, 1] == np.float32(np.sqrt((2 * v0[a] ** 2 + v0[n + a] ** 2) / 3))
        assert np.isnan(f["xi_rhat"][a, 1]) and np.isnan(f["p_gt1"][a, 1]) and np.isnan(f["corr_vh"][a, 1])


def test_quantiles_inside_one_bin():
    """every count in one bin: the quantiles are linear inside it, lo + (b + q) width exactly as the formula gives them"""
    n, nbin, b = 1, 8, 5
    vmin, vmax = np.float32([[3.0], [3.0]]), np.float32([[4.0], [4.0]])
    rs = rr.empty_record(n, 2, 1, nbin)
    rs["xhist"][0, 0, b] = 40
    rs["rsum"][:] = 1.0
    st = dict(sums=np.ones((2, 2, 2)))
    f = rr.final(st, rs, vmin, vmax, np.float32([[3.5], [3.5]]), np.array([0]), 1, 2, 1, 20, nbin)
    lo, hi = (3.0 / 4.0) ** 2, (4.0 / 3.0) ** 2
    for e, qv in enumerate((0.025, 0.5, 0.975)):
        assert f["xi_q"][e, 0, 0] == np.float32(lo + (b + qv * 40 / 40.0) * (hi - lo) / nbin)


def test_linear_gaussian_sampling():
    """The restatement's sample on tests/mc_radial_ref.linear_problem (16 cells, n = 2, 6 + 6 periods, the box 10 sd wide, smooth,
    damp and couple all non-zero, 32 chains, kind 0, 1500 + 4000 steps, one seed) against the analytic posterior (K^T W^2 K + P2)^-1
    and fp64 quadrature of xi under it.  Measured, maxima over cells and knots: |mean - mu| / sd 0.0308, |std / sd - 1| 0.0168,
    |corr - analytic| 0.0217 (analytic 0.137, 0.122), |E xi - quadrature| / sd of xi 0.0261, |std of xi / quadrature - 1| 0.0155,
    |P(xi > 1) - analytic| 0.0063 (analytic 2e-5 .. 1 over the cells); R-hat 1.0037 at most, of xi 1.0027; acceptance 0.27 .. 0.37.
    LINEAR_BARS of tests/mc_radial_ref.py, which the device test shares, are twice these."""
    pb = rr.linear_problem()
    n, ncell, nchain, nbin = pb["n"], pb["ncell"], 32, 64
    assert ((pb["vmax"] - pb["vmin"]).astype(np.float64) >= 8 * pb["sd"]).all() and (pb["vmin"] > 0).all()
    nburn, nsample = rr.LINEAR_STEPS
    kmax = pb["kr"] + pb["kl"]
    wdat = np.full((kmax, ncell), pb["w"], np.float32)
    vref = np.full((2 * n, ncell), 3.5, np.float32)
    st, tp, ns, rs = rr.sample(lambda v: pb["KR"] @ v[:n].astype(np.float64), lambda v: pb["KL"] @ v[:n].astype(np.float64), nburn, nsample,
                               50, np.arange(ncell), nchain, pb["vmin"].T.copy(), pb["vmax"].T.copy(), np.full(ncell, 3.5, np.float32),
                               pb["cobs"].T.copy(), wdat, nbin, 77, pb["couple"], prior=(pb["smooth"], pb["damp"], vref))
    vel0 = np.full((2 * n, ncell), 3.5, np.float32)
    r = rr.mc_ref.final(st, pb["vmin"].T.copy(), pb["vmax"].T.copy(), vel0, np.arange(ncell), ncell, nchain, 1, nsample, nsample, nbin)
    f = rr.final(st, rs, pb["vmin"].T.copy(), pb["vmax"].T.copy(), vel0, np.arange(ncell), ncell, nchain, 1, nsample, nbin)
    fig = rr.linear_figures(pb, r["mean"].T, r["std"].T, f["corr_vh"].T, f["xi_mean"].T, f["xi_std"].T, f["p_gt1"].T)
    print(f"\n[measured] R-hat max {r['rhat'].max():.4f}, of xi {f['xi_rhat'].max():.4f}; acceptance {r['accept'].min():.3f}.."
          f"{r['accept'].max():.3f}; posterior sd {pb['sd'].min():.4f}..{pb['sd'].max():.4f} km/s, corr {pb['corr']}, P(xi > 1) "
          f"{pb['p_gt1'].min():.3f}..{pb['p_gt1'].max():.3f}")
    for k, v in fig.items():
        within(f"restatement against the analytic posterior, {k}", v, rr.LINEAR_BARS[k])
    assert r["rhat"].max() < 1.05 and f["xi_rhat"].max() < 1.05
