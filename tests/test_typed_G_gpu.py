"""-m gpu: the code behind the typed dispersion tables is blind to the wave type.  The tables of the common model
(tests/typed_kernels_ref.py, the two columns whose Love curves end left as drawn: a map with a zero velocity cannot be ray-traced) go
through dazim_fmm_batch and dazim_rays_build_G with K = 11 virtual periods on a 5 x 4 geometry, 3 sources x 4 receivers per virtual
period.  Each segment's rows are bit-equal, values and columns, to the rows of a call that is given only that segment's slice of the
tables with its periods renumbered from 1; and a row of a Love segment carries no Vp contribution: with the Vs and rho kernels
zeroed, every entry of it is 0."""
import numpy as np
import pytest

from tests import synth
from tests import typed_kernels_ref as T

pytestmark = pytest.mark.gpu

GEO = (T.NX, T.NY, 30.0, 100.0, 0.25, 0.25)
NSRC, NRCV = 3, 4
OFF, K = T.offsets(T.SEGMENTS)


def rays(kmax):
    """period -> source -> receiver: (scx, scz, period_idx, field_of_ray, rcx, rcz); stations 0..2 are the sources, 3..6 the receivers"""
    lat, lon = synth.stations(T.NX, T.NY, *GEO[2:], NSRC + NRCV, seed=5, shrink=0.05)
    sx, sz = synth.radians(lat, lon)
    scx, scz = np.tile(sx[:NSRC], kmax), np.tile(sz[:NSRC], kmax)
    per = np.repeat(np.arange(1, kmax + 1, dtype=np.int32), NSRC)
    ray_f = np.repeat(np.arange(kmax * NSRC, dtype=np.int32), NRCV)
    return scx, scz, per, ray_f, np.tile(sx[NSRC:], kmax * NSRC), np.tile(sz[NSRC:], kmax * NSRC)


def rows_of(ctx, vel, pv, sen):
    """(irow, icol, rw, tpred) of the G rows over the tables pv [k][ncol], sen 3 x [nz][k][ncol]"""
    scx, scz, per, ray_f, rx, rz = rays(pv.shape[0])
    fields = ctx.fmm_batch(*GEO, pv, scx, scz, per)
    G, tpred, _ = ctx.rays_build_G(*GEO, vel, fields, scx, scz, per, ray_f, rx, rz, sen)
    ir, ic, rw = G.to_coo()
    G.free()
    return ir, ic, rw, tpred


@pytest.fixture(scope="module")
def tables(ctx):
    vel = T.common_model(ended=False)
    pv, sen, nf = ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS, T.SUBLAYERS)
    assert nf == 0 and pv.shape[0] == K == 11
    return vel, pv, sen


def test_each_segments_rows_are_the_rows_of_its_slice_alone(ctx, tables):
    vel, pv, sen = tables
    ir, ic, rw, tpred = rows_of(ctx, vel, pv, sen)
    per_k = NSRC * NRCV
    assert len(tpred) == K * per_k and len(rw) > 0
    for (iw, ig, t), o in zip(T.SEGMENTS, OFF):
        a, b = o, o + len(t)
        ir_s, ic_s, rw_s, tp_s = rows_of(ctx, vel, np.ascontiguousarray(pv[a:b]), [np.ascontiguousarray(s[:, a:b]) for s in sen])
        sel = (ir > a * per_k) & (ir <= b * per_k)
        assert sel.sum() == len(rw_s) > 0, (iw, ig)
        assert np.array_equal(ir[sel] - a * per_k, ir_s) and np.array_equal(ic[sel], ic_s) and np.array_equal(rw[sel], rw_s), (iw, ig)
        assert np.array_equal(tpred[a * per_k:b * per_k], tp_s), (iw, ig)


def test_love_rows_carry_no_vp_contribution(ctx, tables):
    vel, pv, sen = tables
    zero = np.zeros_like(sen[0])
    ir, ic, rw, _ = rows_of(ctx, vel, pv, [zero, sen[1], zero])
    love = ir > OFF[2] * NSRC * NRCV
    assert not rw[love].any()
    assert (rw[~love] != 0).mean() > 0.9          # (the Rayleigh rows do)
