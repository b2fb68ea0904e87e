"""CPU: the restatement of the Monte-Carlo step with the Gaussian smoothness prior (tests/mc_prior_ref.py) before the device is
involved: with the prior off it is tests/mc_ref.py's step in every mode, its Q is d^T P d of a densely built P, and the library
exports the two calls of the prior."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_prior_ref, mc_ref


def same(a, b, where):
    """two results of a step, field by field: arrays by their bytes"""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], where + (k,))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


@pytest.mark.parametrize("noise", [0, 1])
@pytest.mark.parametrize("ntemp", [1, 4])
@pytest.mark.parametrize("kind", [0, 1])
def test_no_prior_is_mc_ref(kind, ntemp, noise):
    """3 cells x 8 chains, 3 knots, 5 periods, 16 burn-in steps (adaptation every 3) and 4 recorded ones on random curves, some
    without a root: the two restatements side by side from one state, every returned field equal at every step; kind 1 factors"""
    rng = np.random.default_rng(100 + 4 * kind + 2 * (ntemp > 1) + noise)
    ncs, nchain, nlay, kmax, nbin, seed, nadapt, nburn, nrec = 3, 8, 3, 5, 16, 0xABCDEF0123, 3, 16, 4
    ncol = ncs * nchain
    gcell = np.array([0, 2, 5])
    rep = lambda x: np.repeat(x, nchain, axis=-1)
    vmin = rng.uniform(2.8, 3.4, (nlay, ncs)).astype(np.float32)
    vmax = (vmin + rng.uniform(0.3, 1.2, vmin.shape)).astype(np.float32)
    lo, hi = rep(vmin.astype(np.float64)), rep(vmax.astype(np.float64))
    cb = rep(rng.uniform(3.2, 4.0, (kmax, ncs)).astype(np.float32))
    wdat = rng.uniform(50, 150, (kmax, ncs)).astype(np.float32)
    wdat[1, 0] = 0.0
    wd = rep(wdat)
    _, _, _, gid = mc_ref.layout(ncol, nchain, ntemp, gcell)
    prop = np.concatenate([mc_ref.start_models(gid, lo, hi, seed), np.full((1, ncol), 4.4, np.float32)])
    st = dict(cur=prop.copy(), chi2=np.full(ncol, np.inf), scale=np.full(ncs, 0.05, np.float32), step=0,
              sums=np.zeros((2, nlay, ncol)), hist=np.zeros((ncs, nlay, nbin), np.uint32), accepted=np.zeros(ncol, np.int64),
              best=np.zeros((nlay, ncs), np.float32), best_chi2=np.full(ncs, np.inf))
    tp = dict(ntemp=ntemp, tmax=16.0, nswap=1)
    if ntemp > 1:
        tp.update(beta=mc_ref.ladder(ntemp, 16.0), scale=np.full((ncs, ntemp), 0.05, np.float32),
                  swap_try=np.zeros((ncs, ntemp - 1), np.int64), swap_acc=np.zeros((ncs, ntemp - 1), np.int64))
    tp = mc_ref.ladder_state(st, tp)
    cov = mc_ref.empty_cov(ncs, nlay) if kind == 1 else None
    ns = mc_ref.empty_noise(0.25, 0.5, ncol) if noise else None
    acc_win = np.zeros((ncs, ntemp), np.int64)
    nbd = nfact = ndec = nswapped = 0
    for t in range(1, nburn + nrec + 1):
        record = t > nburn
        adapt = False
        if not record and t > 1:
            nbd += 1
            adapt = nbd % nadapt == 0
        pv = (cb.astype(np.float64) + rng.normal(0, 0.012, cb.shape)).astype(np.float32).astype(np.float64)
        pv[rng.random(pv.shape) < (0.1 if t <= 2 else 0.01)] = 0.0
        args = (prop, pv, t, record, adapt, nadapt, acc_win, gcell, nchain, lo, hi, cb, wd, nbin, seed)
        a = mc_ref.step(st, tp, cov, ns, *args)
        b = mc_prior_ref.step(st, tp, cov, ns, None, *args)
        assert b[8] is None and b[9] == dict(dec=0, swap=0)
        for i, (x, y) in enumerate(zip(a, b[:8])):
            if x is None or y is None:
                assert x is None and y is None, (t, i)
            else:
                same(x, y, (t, i))
        st, tp, cov, ns, acc, acc_win, factored, _ = a
        nfact += len(factored)
        ndec += int(acc.sum()) if t > 1 else 0
        prop = mc_ref.proposals(st["cur"], tp["scale"], cov, prop, t, gcell, nchain, lo, hi, seed)
    nswapped = int(tp["swap_acc"].sum())
    assert ndec > 0 and st["hist"].sum() == nrec * nlay * ncs * (nchain // ntemp)
    assert nfact > 0 if kind == 1 else nfact == 0
    assert nswapped > 0 if ntemp > 1 else nswapped == 0
    if noise:
        assert ns["ncnt"].sum() > 0


def dense_precision(n, smooth, damp):
    """P = smooth^2 L^T L + damp^2 I with L written row by row: 2 on the diagonal, -1 beside it in every row but the first and the
    last"""
    L = np.zeros((n, n))
    for i in range(n):
        L[i, i] = 2.0
        if 0 < i < n - 1:
            L[i, i - 1] = -1.0
            L[i, i + 1] = -1.0
    return smooth ** 2 * (L.T @ L) + damp ** 2 * np.eye(n)


@pytest.mark.parametrize("nlay", [1, 2, 3, 7])
def test_q_is_the_quadratic_form(nlay):
    """Q of 50 random columns against d^T P d to 1e-12 relative, with both terms, the smoothing alone and the damping alone"""
    rng = np.random.default_rng(nlay)
    v = rng.uniform(2.5, 4.5, (nlay, 50)).astype(np.float32)
    vref = rng.uniform(3.0, 4.0, (nlay, 50)).astype(np.float32)
    d = v.astype(np.float64) - vref.astype(np.float64)
    for smooth, damp in ((2.0, 0.5), (3.0, 0.0), (0.0, 1.5)):
        P = dense_precision(nlay, smooth, damp)
        want = np.einsum("ac,ab,bc->c", d, P, d)
        got = mc_prior_ref.prior_q(v, vref, smooth, damp)
        assert (want > 0).all()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (nlay, smooth, damp)
        assert (np.abs(got - want) <= 1e-12 * want).all(), (nlay, smooth, damp)


def test_library_exports_the_prior_calls():
    dz.build()
    lib = dz.load()
    for name in ("dazim_mc_set_prior", "dazim_mc_prior_state"):
        assert hasattr(lib, name), name
