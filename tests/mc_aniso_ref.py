"""NumPy fp64 restatement of the Gc/Gs sample (dazim_mc_aniso_step) and of its statistics (dazim_mc_aniso_result), written from the
text of include/dazim.h.  The solve and the inverse are numpy.linalg's, so the restatement does not share the kernel's elimination
order: the comparison is between two factorisations of the same matrix."""
import numpy as np


def ltl(n):
    """L^T L of the depth rule of dazim_column_lsq on one column of n knots: first and last row the single entry 2, an inner row
    2, -1, -1"""
    L = np.zeros((n, n))
    for i in range(n):
        L[i, i] = 2.0
        if 0 < i < n - 1:
            L[i, i - 1] = L[i, i + 1] = -1.0
    return L.T @ L


def normal_matrix(K, w, smooth, damp):
    """A = K^T W^2 K + smooth^2 L^T L + damp^2 I for K [kmax][nlay] and w [kmax] (fp32 values, squared in fp64)"""
    K = np.asarray(K, np.float64)
    w2 = np.asarray(w, np.float32).astype(np.float64) ** 2
    n = K.shape[1]
    s2, d2 = np.float64(np.float32(smooth)) ** 2, np.float64(np.float32(damp)) ** 2
    return K.T @ (w2[:, None] * K) + s2 * ltl(n) + d2 * np.eye(n)


def conditional(K, w, r, smooth, damp):
    """the Gaussian of Gc/Gs given one Vs column: x^ [2][nlay] and diag C [nlay]"""
    K = np.asarray(K, np.float64)
    w2 = np.asarray(w, np.float32).astype(np.float64) ** 2
    A = normal_matrix(K, w, smooth, damp)
    b = K.T @ (w2[None, :] * np.asarray(r, np.float32).astype(np.float64)).T      # [nlay][2]
    return np.linalg.solve(A, b).T, np.diag(np.linalg.inv(A)).copy()


def new_state(nlay, ncolc):
    return dict(asum=np.zeros((5, nlay, ncolc)), avar=np.zeros((nlay, ncolc)), acnt=np.zeros(ncolc, np.int64), skipped=0)


def step(st, lsen, chi2_cold, cell_of_col, amap, wa, smooth, damp):
    """one sample: lsen [nlay][kmax][ncolc], chi2_cold [ncolc] the chi^2 of the cold columns' chains, cell_of_col [ncolc] the inner
    cell of each cold column, amap [2][kmax][ncell], wa [kmax][ncell].  st is changed in place and returned."""
    nlay, kmax, ncolc = lsen.shape
    for col in range(ncolc):
        if np.isinf(chi2_cold[col]):
            st["skipped"] += 1
            continue
        cell = cell_of_col[col]
        x, dg = conditional(lsen[:, :, col].T, wa[:, cell], amap[:, :, cell], smooth, damp)
        st["asum"][0, :, col] += x[0]
        st["asum"][1, :, col] += x[1]
        st["asum"][2, :, col] += x[0] * x[0]
        st["asum"][3, :, col] += x[1] * x[1]
        st["asum"][4, :, col] += x[0] * x[1]
        st["avar"][:, col] += dg
        st["acnt"][col] += 1
    return st


def result(st, cells, ncell, ncold):
    """the statistics per inner cell: cells [ncs] = the inner cell of each sampled cell; returns dict mean, std, std_between
    [2][nlay][ncell], cov_cs [nlay][ncell] (fp32) and nsamp [ncell]"""
    nlay = st["avar"].shape[0]
    mean = np.zeros((2, nlay, ncell), np.float32)
    std = np.zeros((2, nlay, ncell), np.float32)
    stdb = np.zeros((2, nlay, ncell), np.float32)
    cov = np.zeros((nlay, ncell), np.float32)
    nsamp = np.zeros(ncell, np.int64)
    for cs, cell in enumerate(cells):
        sl = slice(cs * ncold, (cs + 1) * ncold)
        n = int(st["acnt"][sl].sum())
        nsamp[cell] = n
        if n == 0:
            std[:, :, cell] = stdb[:, :, cell] = np.nan
            cov[:, cell] = np.nan
            continue
        S = np.zeros((5, nlay))
        Sv = np.zeros(nlay)
        for g in range(cs * ncold, (cs + 1) * ncold):      # in column order, as the kernel's lane
            S += st["asum"][:, :, g]
            Sv += st["avar"][:, g]
        m = S[:2] / n
        between = np.maximum(S[2:4] / n - m * m, 0.0)
        within = Sv / n
        mean[:, :, cell] = m
        std[:, :, cell] = np.sqrt(within[None, :] + between)
        stdb[:, :, cell] = np.sqrt(between)
        cov[:, cell] = S[4] / n - m[0] * m[1]
    return dict(mean=mean, std=std, std_between=stdb, cov_cs=cov, nsamp=nsamp)
