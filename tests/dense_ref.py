"""What the fp64 restatements of the posterior and trade-off entries share (map_posterior_ref, model_posterior_ref, column_res_ref,
map_tradeoff_ref, model_tradeoff_ref): the dense route of the kernels (right-looking Cholesky, M = R^-1 by forward substitution,
C = M^T M in ascending order), what is summed along a row of Rm, and the comparison of a call's outputs with a reference."""
import numpy as np


def cholesky(A):
    """R with A = R R^T (lower triangle) by the right-looking Cholesky, column by column; None at a pivot that is not finite and > 0"""
    R = np.tril(A)
    for c in range(len(R)):
        if not (np.isfinite(R[c, c]) and R[c, c] > 0):
            return None
        R[c, c] = np.sqrt(R[c, c])
        R[c + 1:, c] /= R[c, c]
        R[c + 1:, c + 1:] -= np.tril(np.outer(R[c + 1:, c], R[c + 1:, c]))
    return R


def inverse_factor(R):
    """M = R^-1, row by row (forward substitution on every unit vector)"""
    n = len(R)
    M = np.zeros((n, n))
    for i in range(n):
        M[i, :i + 1] = ((np.arange(i + 1) == i) - R[i, :i] @ M[:i, :i + 1]) / R[i, i]
    return M


def gram_of_inverse(M):
    """C = M^T M as C_ac = sum_{i >= max(a, c)} M_ia M_ic, ascending i"""
    n = len(M)
    C = np.zeros((n, n))
    for i in range(n):
        C[:i + 1, :i + 1] += np.outer(M[i, :i + 1], M[i, :i + 1])
    return C


def per_unknown(C, Rm, blk, ci, cj, z=None):
    """what the row pass writes per unknown a from row a of Rm and of C: std_post, std_noise, rdiag, rsum, width_h, leak, and width_z
    where z is given; blk, ci, cj, z the block, the two horizontal cell indices and the depth of every unknown"""
    dist2 = lambda u: (u[None, :] - u[:, None]) ** 2
    same = blk[None, :] == blk[:, None]
    sq = Rm ** 2
    own, alls = (sq * same).sum(axis=1), sq.sum(axis=1)
    width = lambda d2: np.where(own > 0, np.sqrt((sq * same * d2).sum(axis=1) / np.where(own > 0, own, 1.0)), 0.0)
    out = dict(std_post=np.sqrt(np.diag(C)), std_noise=np.sqrt(np.maximum(np.einsum("ac,ca->a", Rm, C), 0.0)), rdiag=np.diag(Rm).copy(),
               rsum=Rm.sum(axis=1), width_h=width(dist2(ci) + dist2(cj)),
               leak=np.where(alls > 0, (sq * ~same).sum(axis=1) / np.where(alls > 0, alls, 1.0), 0.0))
    if z is not None:
        out["width_z"] = width(dist2(z))
    return out


def worst(got, ref, keys, reshaped=()):
    """per output max |got - ref| / max(1, max |ref|) over the finite reference values; NaN must sit where the reference has NaN, None
    where it has None, and the shapes agree but for the outputs named in `reshaped`, which the reference keeps in another layout"""
    res = {}
    for k in keys:
        if ref[k] is None:
            assert got[k] is None, k
            continue
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        if k in reshaped:
            g = g.reshape(r.shape)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        bad = np.isnan(r)
        assert np.array_equal(np.isnan(g), bad), k
        res[k] = float(np.abs(g - r)[~bad].max() / max(1.0, np.abs(r[~bad]).max())) if (~bad).any() else 0.0
    return res
