"""The NumPy restatement of the Gc/Gs sums (tests/mc_aniso_ref.py) against what it must reduce to: with one K for every sample the
ridge solution and the diagonal of the inverse normal matrix, with two K in equal numbers the law of total variance evaluated directly."""
import numpy as np

from tests import mc_aniso_ref as ref


def problem(rng, nlay, kmax):
    dep = np.arange(nlay)[None, :]
    per = np.arange(kmax)[:, None]
    K = (0.02 * np.exp(-0.5 * ((dep - per * nlay / kmax) / 1.5) ** 2) * (1 + 0.2 * rng.random((kmax, nlay)))).astype(np.float32)
    w = rng.uniform(50, 150, kmax).astype(np.float32)
    w[1] = 0.0
    r = rng.normal(0, 0.02, (2, kmax)).astype(np.float32)
    return K, w, r


def test_one_kernel_is_the_ridge_solution():
    rng = np.random.default_rng(2)
    nlay, kmax, ncold, nsmp = 6, 9, 4, 3
    K, w, r = problem(rng, nlay, kmax)
    smooth, damp = 0.3, 0.1
    lsen = np.repeat(K.T[:, :, None], ncold, axis=2)
    amap, wa = r[:, :, None], w[:, None]
    st = ref.new_state(nlay, ncold)
    for _ in range(nsmp):
        ref.step(st, lsen, np.zeros(ncold), np.zeros(ncold, int), amap, wa, smooth, damp)
    assert st["skipped"] == 0 and (st["acnt"] == nsmp).all()
    res = ref.result(st, [0], 1, ncold)
    # the ridge solution from the stacked least-squares problem, not the normal equations
    L = np.linalg.cholesky(ref.ltl(nlay)).T
    w64 = w.astype(np.float64)
    G = np.vstack([w64[:, None] * K.astype(np.float64), np.float64(np.float32(smooth)) * L, np.float64(np.float32(damp)) * np.eye(nlay)])
    for e in range(2):
        d = np.concatenate([w64 * r[e].astype(np.float64), np.zeros(2 * nlay)])
        x = np.linalg.lstsq(G, d, rcond=None)[0]
        assert np.allclose(res["mean"][e, :, 0], x, rtol=1e-5, atol=1e-9)
    C = np.linalg.inv(G.T @ G)
    assert np.allclose(res["std"][:, :, 0] ** 2, np.diag(C)[None, :], rtol=1e-5)
    # equal samples: the spread between them is rounding only
    assert (res["std_between"] <= 1e-6 * np.abs(res["mean"]).max()).all()
    assert res["nsamp"][0] == nsmp * ncold


def test_two_kernels_total_variance():
    rng = np.random.default_rng(3)
    nlay, kmax, ncold = 5, 8, 6
    K1, w, r = problem(rng, nlay, kmax)
    K2 = (K1 * (1 + 0.3 * rng.random(K1.shape))).astype(np.float32)
    smooth, damp = 0.2, 0.05
    lsen = np.stack([(K1 if g % 2 == 0 else K2).T for g in range(ncold)], axis=2)
    st = ref.new_state(nlay, ncold)
    chi2 = np.zeros(ncold)
    for _ in range(2):
        ref.step(st, lsen, chi2, np.zeros(ncold, int), r[:, :, None], w[:, None], smooth, damp)
    res = ref.result(st, [0], 1, ncold)
    x1, c1 = ref.conditional(K1, w, r, smooth, damp)
    x2, c2 = ref.conditional(K2, w, r, smooth, damp)
    mean = 0.5 * (x1 + x2)
    var = 0.5 * (c1 + c2)[None, :] + 0.25 * (x1 - x2) ** 2          # E[C] + Var[x^] of a fair two-point mixture
    assert np.allclose(res["mean"][:, :, 0], mean, rtol=1e-6, atol=1e-12)
    assert np.allclose(res["std"][:, :, 0] ** 2, var, rtol=1e-5)
    assert np.allclose(res["std_between"][:, :, 0], 0.5 * np.abs(x1 - x2), rtol=1e-4, atol=1e-9)
    assert np.allclose(res["cov_cs"][:, 0], 0.25 * (x1[0] - x2[0]) * (x1[1] - x2[1]), rtol=1e-4, atol=1e-12)
    assert (res["std_between"] > 0).any()


def test_skipped_and_empty():
    rng = np.random.default_rng(4)
    nlay, kmax, ncold = 3, 4, 2
    K, w, r = problem(rng, nlay, kmax)
    lsen = np.repeat(K.T[:, :, None], 2 * ncold, axis=2)
    st = ref.new_state(nlay, 2 * ncold)
    chi2 = np.array([0.0, np.inf, np.inf, np.inf])
    amap = np.repeat(r[:, :, None], 3, axis=2)
    wa = np.repeat(w[:, None], 3, axis=1)
    ref.step(st, lsen, chi2, np.array([0, 0, 2, 2]), amap, wa, 0.1, 0.1)
    assert st["skipped"] == 3 and st["acnt"].tolist() == [1, 0, 0, 0]
    res = ref.result(st, [0, 2], 3, ncold)
    assert res["nsamp"].tolist() == [1, 0, 0]
    assert (res["mean"][:, :, 1] == 0).all() and (res["std"][:, :, 1] == 0).all()          # a cell without Vs data
    assert (res["mean"][:, :, 2] == 0).all() and np.isnan(res["std"][:, :, 2]).all() and np.isnan(res["cov_cs"][:, 2]).all()
