"""CPU: the restatement of the Gaussian smoothness prior (tests/mc_prior_ref.py) before the device is involved: its Q is d^T P d of
a densely built P, and the library exports the two calls of the prior."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests import mc_prior_ref


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
