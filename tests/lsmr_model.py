"""A plain NumPy / SciPy statement of LSMR as the reference runs it (inv/lsmrModule.f90:36-750, with localVEnqueue and
localVOrtho: modified Gram-Schmidt against a ring of the last localSize v) -- TEST INFRASTRUCTURE ONLY.

`lsmr_model(A, b, ..., T)` keeps every vector and every scalar recurrence in the type T and takes every norm and every dot
product as an fp64 sum rounded to T once.  Two uses:

  T = float64   the yardstick: LSMR in fp64.
  T = float32   the library's precision contract (fp32 vectors and recurrences, fp64 sums): what the device's arithmetic can
                be expected to stay with, and how far that arithmetic leaves fp64 by itself.

The products A v and A^T u are SciPy's CSR products in T (a row's terms are summed in T, in column order).  One record per
iteration comes back: the norms, the three tests, rtol, the decision, and x where asked for.  tests/test_lsmr_model_cpu.py pins
this file against numpy.linalg.lstsq and the oracle (oracle/lsmr.c)."""
import numpy as np
import scipy.sparse as sp


def coo_to_csr(m, n, irow, icol, rw):
    """the 1-based COO triplets the library and the oracle take -> scipy CSR in fp64 (duplicates summed)"""
    return sp.csr_matrix((np.asarray(rw, np.float64), (np.asarray(irow) - 1, np.asarray(icol) - 1)), shape=(m, n))


def _nrm2(x, T):
    x64 = x.astype(np.float64, copy=False)
    return T(np.sqrt(np.dot(x64, x64)))


def _d2norm(a, b, T):   # :708-721
    scale = abs(a) + abs(b)
    if scale == 0:
        return T(0)
    return T(scale * np.sqrt((a / scale) * (a / scale) + (b / scale) * (b / scale)))


def decide(itn, itnlim, test1, test2, test3, t1, rtol, atol, ctol, T=np.float32):
    """the stopping rules in the reference's order (:595-616): the last one that holds wins, so 1 beats 2 beats ... 7.
    t1 = None leaves rule 4 out (a trace record does not carry normx)."""
    one = T(1)
    istop = 0
    if itn >= itnlim: istop = 7
    if one + T(test3) <= one: istop = 6
    if one + T(test2) <= one: istop = 5
    if t1 is not None and one + T(t1) <= one: istop = 4
    if T(test3) <= T(ctol): istop = 3
    if T(test2) <= T(atol): istop = 2
    if T(test1) <= T(rtol): istop = 1
    return istop


def lsmr_model(A, b, damp, atol, btol, conlim, itnlim, localSize, T=np.float64, keep_x=(), stop=True):
    """-> x, info (istop, itn, normA, condA, normr, normAr, normx, as the library's info dict), records.
    records[k - 1] belongs to iteration k: dict(itn, normr, normAr, normA, condA, normx, test1, test2, test3, rtol, istop
    (before the damp remap of 2 to 3), and x where k is in keep_x or keep_x is True).
    stop = False: only itnlim ends the iteration (the records still say what the rules decided), for the iterates behind the
    point where a rule with zero tolerances (4, 5, 6) would have stopped this arithmetic."""
    err = np.seterr(all="ignore")   # (0 / 0 in test2 once normr is 0, as in the reference)
    try:
        return _lsmr(A, b, damp, atol, btol, conlim, itnlim, localSize, T, keep_x, stop)
    finally:
        np.seterr(**err)


def _lsmr(A, b, damp, atol, btol, conlim, itnlim, localSize, T, keep_x, stop):
    A = sp.csr_matrix(A, dtype=T)
    At = sp.csr_matrix(A.T, dtype=T)
    m, n = A.shape
    damp, atol, btol, conlim = T(damp), T(atol), T(btol), T(conlim)
    one, zero = T(1), T(0)
    localVecs = min(int(localSize), m, n)
    x = np.zeros(n, T)
    u = np.array(b, T)
    v = np.zeros(n, T)
    records = []
    info = dict(istop=0, itn=0, normA=zero, condA=zero, normr=zero, normAr=zero, normx=zero)
    alpha, beta = zero, _nrm2(u, T)
    if beta > 0:
        u = (one / beta) * u
        v = At @ u
        alpha = _nrm2(v, T)
    if alpha > 0:
        v = (one / alpha) * v
    normAr = T(alpha * beta)
    info["normAr"] = normAr
    if normAr == 0:
        return x, info, records
    localOrtho, localPointer, localVQueueFull = localVecs > 0, 0, False
    if localOrtho:
        localPointer = 1
        localV = np.zeros((localVecs, n), T)
        localV[0] = v
    zetabar, alphabar, rho, rhobar, cbar, sbar = T(alpha * beta), alpha, one, one, one, zero
    h = v.copy()
    hbar = np.zeros(n, T)
    betadd, betad, rhodold, tautildeold, thetatilde, zeta, d = beta, zero, one, zero, zero, zero, zero
    normA2, maxrbar, minrbar, normb = T(alpha * alpha), zero, T(1e30), beta
    ctol = one / conlim if conlim > 0 else zero
    itn, istop = 0, 0
    while True:
        itn += 1
        u = A @ v - alpha * u
        beta = _nrm2(u, T)
        if beta > 0:
            u = (one / beta) * u
            if localOrtho:   # localVEnqueue :723-731
                if localPointer < localVecs:
                    localPointer += 1
                else:
                    localPointer, localVQueueFull = 1, True
                localV[localPointer - 1] = v
            v = At @ u - beta * v
            if localOrtho:   # localVOrtho :733-748
                for q in range(localVecs if localVQueueFull else localPointer):
                    lv = localV[q]
                    dd = T(np.dot(v.astype(np.float64, copy=False), lv.astype(np.float64, copy=False)))
                    v = v - dd * lv
            alpha = _nrm2(v, T)
            if alpha > 0:
                v = (one / alpha) * v
        alphahat = _d2norm(alphabar, damp, T)
        chat, shat = alphabar / alphahat, damp / alphahat
        rhoold = rho
        rho = _d2norm(alphahat, beta, T)
        c, s = alphahat / rho, beta / rho
        thetanew = s * alpha
        alphabar = c * alpha
        rhobarold, zetaold = rhobar, zeta
        thetabar, rhotemp = sbar * rho, cbar * rho
        rhobar = _d2norm(cbar * rho, thetanew, T)
        cbar = cbar * rho / rhobar
        sbar = thetanew / rhobar
        zeta = cbar * zetabar
        zetabar = -sbar * zetabar
        hbar = h - (thetabar * rho / (rhoold * rhobarold)) * hbar
        x = x + (zeta / (rho * rhobar)) * hbar
        h = v - (thetanew / rho) * h
        betaacute, betacheck = chat * betadd, -shat * betadd
        betahat = c * betaacute
        betadd = -s * betaacute
        thetatildeold = thetatilde
        rhotildeold = _d2norm(rhodold, thetabar, T)
        ctildeold, stildeold = rhodold / rhotildeold, thetabar / rhotildeold
        thetatilde = stildeold * rhobar
        rhodold = ctildeold * rhobar
        betad = -stildeold * betad + ctildeold * betahat
        tautildeold = (zetaold - thetatildeold * tautildeold) / rhotildeold
        taud = (zeta - thetatilde * tautildeold) / rhodold
        d = d + betacheck * betacheck
        normr = T(np.sqrt(d + (betad - taud) * (betad - taud) + betadd * betadd))
        normA2 = normA2 + beta * beta
        normA = T(np.sqrt(normA2))
        normA2 = normA2 + alpha * alpha
        maxrbar = max(maxrbar, rhobarold)
        if itn > 1:
            minrbar = min(minrbar, rhobarold)
        condA = max(maxrbar, rhotemp) / min(minrbar, rhotemp)
        normAr = abs(zetabar)
        normx = _nrm2(x, T)
        test1, test2, test3 = normr / normb, normAr / (normA * normr), one / condA
        t1 = test1 / (one + normA * normx / normb)
        rtol = btol + atol * normA * normx / normb
        istop = decide(itn, itnlim, test1, test2, test3, t1, rtol, atol, ctol, T)
        assert all(type(q) is T for q in (normr, normAr, normA, condA, normx, test1, test2, test3, rtol)), "a scalar left the type T"
        rec = dict(itn=itn, normr=normr, normAr=normAr, normA=normA, condA=condA, normx=normx, test1=test1, test2=test2,
                   test3=test3, rtol=rtol, istop=istop)
        if keep_x is True or (keep_x is not False and itn in keep_x):
            rec["x"] = x.copy()
        records.append(rec)
        if istop != 0 and (stop or itn >= itnlim):
            break
    if damp > 0 and istop == 2:
        istop = 3   # :686
    info = dict(istop=istop, itn=itn, normA=normA, condA=condA, normr=normr, normAr=normAr, normx=normx)
    return x, info, records
