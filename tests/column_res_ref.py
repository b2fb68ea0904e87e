"""NumPy fp64 statements of dazim_column_resolution: `route` follows the kernel (Cholesky of the normal matrix,
the inverse factor column by column, C = M^T M, Rm = I - C P, the noise variance as sum_p w_p^2 (C k_p)^2), `linalg` is
the independent reference (numpy.linalg.inv(A), inv(A) @ K^T W^2 K and, for the noise term, numpy.linalg.solve(A, K^T W)).  Both take one cell; `per_cell` runs either over the inner
cells of a kernel table laid out as dazim_column_lsq reads it."""
import numpy as np

from tests import dense_ref
from tests.test_column_lsq_gpu import depth_rule

OUTPUTS = ("std_post", "std_noise", "rdiag", "rsum", "width", "rows", "trace")


def knot_depths(n):
    """knots that grow apart with depth, as a depth grid does (km, fp32)"""
    k = np.arange(n)
    return (k * (1.0 + 0.1 * k)).astype(np.float32)


def penalty(n, smooth, damp):
    """P = smooth^2 L^T L + damp^2 I with the regularisers rounded to fp32 first, as the C entry receives them"""
    s, d = float(np.float32(smooth)), float(np.float32(damp))
    L = depth_rule(n)
    return s * s * (L.T @ L) + d * d * np.eye(n)


def derived(C, Rm, noise_var, depz):
    n = len(C)
    out = dict(std_post=np.sqrt(np.diag(C)), std_noise=np.sqrt(np.maximum(noise_var, 0.0)), rdiag=np.diag(Rm).copy(),
               rsum=Rm.sum(axis=1), rows=Rm, trace=np.trace(Rm), width=None)
    if depz is not None:
        z = np.asarray(depz, np.float32).astype(np.float64)[:n]
        num = (Rm ** 2 * (z[None, :] - z[:, None]) ** 2).sum(axis=1)
        den = (Rm ** 2).sum(axis=1)
        out["width"] = np.where(den > 0, np.sqrt(num / np.where(den > 0, den, 1.0)), 0.0)
    return out


def route(K, w, smooth, damp, depz=None):
    """the kernel's route on one cell: K [kmax][n], w [kmax]"""
    n = K.shape[1]
    P = penalty(n, smooth, damp)
    A = (K * (w * w)[:, None]).T @ K + P
    R = dense_ref.cholesky(A)
    if R is None:
        return None
    M = dense_ref.inverse_factor(R)
    C = M.T @ M
    Rm = np.eye(n) - C @ P
    # (Rm C)_aa = (C K^T W^2 K C)_aa as the sum of squares sum_p w_p^2 (C k_p)_a^2: the difference C - C P C loses what is small
    return derived(C, Rm, ((K @ C) ** 2 * (w * w)[:, None]).sum(axis=0), depz)


def linalg(K, w, smooth, damp, depz=None):
    n = K.shape[1]
    N = (K * (w * w)[:, None]).T @ K
    C = np.linalg.inv(N + penalty(n, smooth, damp))
    # the noise term from numpy.linalg.solve(A, K^T W), not from inv(A) @ N @ inv(A): inv's error is eps * cond(A) * |C|, and where
    # the data direction is well determined |C k| is far below |C| |k| (nlay 63, one period, smoothing alone: |C| 6.7e3, cond 3e7,
    # std_noise <= 0.13 -- the product form is off by 1.8e-4 there, solve and a long-double Cholesky agree to 3e-11)
    U = np.linalg.solve(N + penalty(n, smooth, damp), K.T * w[None, :])
    return derived(C, C @ N, (U ** 2).sum(axis=1), depz)


def per_cell(fn, nx, ny, nlay, kern, wdat, smooth, damp, depz=None):
    """fn over the inner cells: dict of std_post .. width [nlay][ncell], rows [nlay][nlay][ncell], trace [ncell], all 0 in a cell
    without data, NaN where fn gives up; n_empty and n_failed"""
    kmax = kern.shape[1]
    nvx, ncell = nx - 2, (nx - 2) * (ny - 2)
    w = np.ones((kmax, ncell)) if wdat is None else np.asarray(wdat).reshape(kmax, ncell).astype(np.float64)
    out = {k: np.zeros((nlay, ncell)) for k in ("std_post", "std_noise", "rdiag", "rsum")}
    out["width"] = None if depz is None else np.zeros((nlay, ncell))
    out["rows"], out["trace"] = np.zeros((nlay, nlay, ncell)), np.zeros(ncell)
    out["n_empty"] = out["n_failed"] = 0
    for c in range(ncell):
        if not (w[:, c] != 0).any():
            out["n_empty"] += 1
            continue
        col = (c // nvx + 1) * nx + c % nvx + 1
        K = kern[:nlay, :, col].T.astype(np.float64)
        K[w[:, c] == 0] = 0.0                            # (a period without data is not read)
        one = fn(K, w[:, c], smooth, damp, depz)
        if one is None:
            out["n_failed"] += 1
        for k in OUTPUTS:
            if out[k] is not None:
                out[k][..., c] = np.nan if one is None else one[k]
    return out


def worst(got, ref):
    """per output the largest over the cells of max |got - ref| / max(1, max |ref|), each maximum taken within the cell"""
    res = {}
    for k in OUTPUTS:
        if ref[k] is None:
            continue
        g = np.asarray(got[k], np.float64).reshape(-1, ref[k].shape[-1])
        r = ref[k].reshape(-1, ref[k].shape[-1])
        res[k] = float((np.abs(g - r).max(axis=0) / np.maximum(1.0, np.abs(r).max(axis=0))).max())
    return res
