"""NumPy restatement of the Gaussian smoothness prior of dazim_mc_set_prior (include/dazim.h): Q = s2 |L d|^2
+ d2 |d|^2, the prior energy of a state's knots about the reference, which tests/mc_ref.py's step adds to the energy wherever a
decision is taken, and the prior record."""
import numpy as np


def prior_q(v, vref, smooth, damp):
    """Q of the columns of v [nlay][ncol] fp32 about vref [nlay][ncol] fp32, in the library's order: d = (double)v - (double)vref,
    t_a = 2 d_a at both ends and (2 d_a - d_{a-1}) - d_{a+1} between them, q1 = sum t_a^2 and q2 = sum d_a^2 in knot order from 0.0,
    Q = s2 q1 + d2 q2 with s2, d2 the squares in fp64 of the fp32 smooth and damp"""
    s2 = float(np.float32(smooth)) * float(np.float32(smooth))
    d2 = float(np.float32(damp)) * float(np.float32(damp))
    n = v.shape[0]
    d = v.astype(np.float64) - vref.astype(np.float64)
    q1, q2 = np.zeros(v.shape[1]), np.zeros(v.shape[1])
    for a in range(n):
        t = 2.0 * d[a] if a in (0, n - 1) else (2.0 * d[a] - d[a - 1]) - d[a + 1]
        q1 = q1 + t * t
        q2 = q2 + d[a] * d[a]
    return s2 * q1 + d2 * q2


def empty_prior(smooth, damp, vref, cur):
    """the prior record of a handle whose states are cur [nz][ncol]: vref [nlay][ncol] fp32 per column"""
    nlay = vref.shape[0]
    return dict(smooth=float(np.float32(smooth)), damp=float(np.float32(damp)), vref=vref, q=prior_q(cur[:nlay], vref, smooth, damp))
