"""tests/lsmr_model.py, the NumPy LSMR that tests/test_lsmr_gpu.py measures the device with, pinned on the CPU: the fp64 model against
numpy.linalg.lstsq of the damped system, the mixed model (fp32 vectors and recurrences, fp64 sums) against the oracle."""
import numpy as np
import pytest

from tests.lsmr_model import coo_to_csr, lsmr_model
from tests.test_sparse_gpu import random_system

M, N, DAMP = 90, 40, 0.3


@pytest.fixture(scope="module")
def system():
    irow, icol, rw, m = random_system(M, N, 8, seed=11)
    b = np.random.default_rng(12).standard_normal(m).astype(np.float32)
    A = coo_to_csr(m, N, irow, icol, rw)
    K = np.vstack([A.toarray(), DAMP * np.eye(N)])
    xs = np.linalg.lstsq(K, np.concatenate([b.astype(np.float64), np.zeros(N)]), rcond=None)[0]
    return irow, icol, rw, m, b, A, xs


def test_fp64_model_reaches_the_least_squares_solution(system):
    """n = 40 iterations with a full window span the whole Krylov space: the iterate is the damped least-squares solution"""
    irow, icol, rw, m, b, A, xs = system
    x, info, rec = lsmr_model(A, b, DAMP, 0.0, 0.0, 0.0, N, 100, np.float64)
    assert info["itn"] == N and len(rec) == N
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f"\n[measured] fp64 model vs lstsq after {N} iterations: {err:.3e}")
    assert err <= 1e-12


def test_mixed_model_matches_the_oracle(system, orc):
    irow, icol, rw, m, b, A, xs = system
    cfg = (DAMP, 0.0, 0.0, 0.0, 500, 100)
    x, info, rec = lsmr_model(A, b, *cfg, np.float32)
    xo, io = orc.lsmr(m, N, irow, icol, rw, b, *cfg)
    assert x.dtype == np.float32
    assert (info["istop"], info["itn"]) == (io["istop"], io["itn"])
    for name, xx in (("mixed model", x), ("oracle", xo)):
        err = np.linalg.norm(xx - xs) / np.linalg.norm(xs)
        print(f"\n[measured] {name} vs lstsq, istop {info['istop']} at iteration {info['itn']}: {err:.3e}")
        assert err <= 2e-6
    tol = 1e-6
    for a, c in zip(rec, rec[1:]):
        assert c["normr"] <= a["normr"] * (1 + tol)
        assert c["normAr"] <= a["normAr"] * (1 + tol)
        assert c["normx"] >= a["normx"] * (1 - tol)
        assert a["istop"] == 0
    assert rec[-1]["istop"] != 0 and [r["itn"] for r in rec] == list(range(1, info["itn"] + 1))
