"""-m gpu: the ray kernel's Frechet slots.  A slot (one Frechet grid per lane group of a workgroup, three in joint mode) is all
zeros when a ray starts: the host clears the scratch once per call and every ray puts zeros back into what it wrote.  A batch of
these sizes gives every workgroup one quad of rays at the most, so nothing would see a slot that was left dirty; option rays.nwg
caps the number of workgroups, and with one or two of them every slot serves many rays, one after the other.  The capped calls must
give the bits of the uncapped call (and of tests/golden/rays_step_bits.json) -- predicted times, boundary count, G triplets -- for
every row form on the three batches of tests/rays_step_cases.py (17 x 15 nodes: nvx != nvz, a transposed slot index cannot cancel
out), with a 16-entry cell list (overflow sweep, emit pass retraces), with receivers outside the grid between ordinary rays, for the
dense twin and for rays.keep_small; and calls of different forms and grids on one context must not see each other's scratch."""
import json
import os
import sys

import numpy as np
import pytest

from tests import rays_step_cases as cases
from tests.test_rays_gpu import build_case, flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rays_step_bits as bits   # noqa: E402

pytestmark = pytest.mark.gpu

RPW = 8   # rays per wavefront of the count pass = slots per workgroup


@pytest.fixture(scope="module")
def batches(ctx, orc):
    """inputs and column-major fields of the three batches, once"""
    out = {}
    for name in cases.NAMES:
        inp = bits.inputs(orc, name)
        out[name] = (inp, bits.fields_of(ctx, inp))
    return out


def call(ctx, inp, fields, form, **opts):
    """(tpred, n_boundary, triplets) of one ray call under options `opts` (given as rays_nwg = 1 for rays.nwg = 1)"""
    names = [k.replace("_", ".", 1) for k in opts]
    try:
        for k, v in zip(names, opts.values()):
            ctx.set_option(k, v)
        G, tpred, nb = bits.build(ctx, inp, fields, form)
    finally:
        for k in names:
            ctx.set_option(k, 0)
    res = (np.array(tpred), nb, G.to_coo())
    G.free()
    return res


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("name", cases.NAMES)
def test_slots_that_serve_many_rays(ctx, batches, name):
    inp, fields = batches[name]
    golden = json.load(open(bits.GOLDEN))
    nray = len(inp["flat"][3])
    for form in bits.FORMS:
        free = call(ctx, inp, fields, form)
        assert ctx.stat("rays.nwg") >= (nray + RPW - 1) // RPW - 7            # uncapped: one quad per workgroup (rounded to 8s)
        want = golden[f"{name}.{form}"]
        assert (len(free[0]), len(free[2][2]), free[1]) == (want["m"], want["nnz"], want["n_boundary"]), (name, form)
        assert bits.sha1(free[2], free[0]) == want["sha1"], (name, form)
        for nwg in (1, 2):
            capped = call(ctx, inp, fields, form, rays_nwg=nwg)
            assert ctx.stat("rays.nwg") == nwg and (nray + RPW - 1) // RPW >= 4 * nwg   # every slot is taken again and again
            assert same(capped, free), (name, form, nwg)
            assert bits.sha1(capped[2], capped[0]) == want["sha1"], (name, form, nwg)


def test_slots_that_serve_many_rays_with_a_16_entry_cell_list(ctx, batches):
    """rays.lcap = 16: the lists outgrow the LDS capacity (full-grid sweep of the slot) and the saved lists (the emit pass traces the
    ray again, in a slot of its own pass)"""
    inp, fields = batches["base"]
    for form in bits.FORMS:
        free = call(ctx, inp, fields, form)
        for nwg in (0, 1, 2):
            capped = call(ctx, inp, fields, form, rays_nwg=nwg, rays_lcap=16)
            assert ctx.stat("rays.list_sweeps") > 10 and ctx.stat("rays.list_retraced") > 10
            assert same(capped, free), (form, nwg)


def test_rays_with_a_status_between_ordinary_rays_in_one_slot(ctx, batches):
    """receivers outside the grid: their rays get a status, trace nothing and must leave the slot to the next ray as they found it.
    Such a call fails as a whole (the reference STOPs) and returns no matrix, but it has filled in the other rays' times, the entry
    count of their rows and the boundary count: they must be those of the batch without the outside receivers, with and without the
    cap.  Input order (rays.sort = 0), so that the host knows which rays share a slot: with one workgroup, ray i goes to slot i % 8
    of quad i // 8."""
    import dazimsurftomo_amd as dz
    inp, fields = batches["base"]
    scx, scz, per, ray_f, rx, rz = inp["flat"]
    nray = len(rx)
    bad = np.array([9, 21, 22, 40, 67, 100])
    good = np.setdiff1d(np.arange(nray), bad)
    # host check of the order: every such ray has an ordinary ray before it and after it in its slot
    assert all(b - RPW >= 0 and b + RPW < nray and b - RPW not in bad and b + RPW not in bad for b in bad)
    rx_bad, rz_bad = rx.copy(), rz.copy()
    rx_bad[bad] = np.float32(0.2); rz_bad[bad[::2]] = np.float32(3.0)     # colatitude 11 degrees / longitude 172 degrees: far outside
    try:
        ctx.set_option("rays.sort", 0)
        inp_good = dict(inp, flat=(scx, scz, per, ray_f[good], rx[good], rz[good]))
        G, t_good, nb_good = bits.build(ctx, inp_good, fields, "joint")
        nnz_good = G.nnz
        G.free()
        for nwg in (0, 1, 2):
            ctx.set_option("rays.nwg", nwg)
            with pytest.raises(dz.DazimError) as e:
                bits.build(ctx, dict(inp, flat=(scx, scz, per, ray_f, rx_bad, rz_bad)), fields, "joint")
            assert e.value.code == dz.DAZIM_E_RECEIVER_OUTSIDE
            part = e.value.partial
            assert part["nnz"] == nnz_good and part["n_boundary"] == nb_good, nwg
            assert np.array_equal(np.asarray(part["tpred"])[good], np.asarray(t_good)), nwg
    finally:
        ctx.set_option("rays.sort", 1)
        ctx.set_option("rays.nwg", 0)


def small_case(orc):
    """a smaller grid (12 x 11 nodes) with its own model, stations and dispersion inputs"""
    nx, ny = 12, 11
    vel, *tabs = build_case(nx, ny, cases.DEPZ, cases.KMAX, 7, 4, 5)
    pv, sen = orc.depthkernel(vel, cases.DEPZ, cases.T, cases.MINTHK)
    return nx, ny, vel, pv, sen, flatten(*tabs)


def small_call(c, case):
    nx, ny, vel, pv, sen, (scx, scz, per, ray_f, rx, rz) = case
    fields = c.fmm_batch(nx, ny, cases.GOXD, cases.GOZD, cases.DV, cases.DV, pv, scx, scz, per)
    G, tpred, nb = c.rays_build_G(nx, ny, cases.GOXD, cases.GOZD, cases.DV, cases.DV, vel, fields, scx, scz, per, ray_f, rx, rz, sen)
    res = (np.array(tpred), nb, G.to_coo())
    G.free()
    return res


def test_stale_scratch_across_calls_on_one_context(ctx, orc, batches):
    """the slot scratch is one block cached by name: map rows (three grids per slot), joint and iso rows on one grid, then iso rows
    on a smaller grid (other slot size: its slots straddle the earlier ones) and on the first grid again -- every call as on a
    context that has never made another"""
    import dazimsurftomo_amd as dz
    inp, fields = batches["base"]
    small = small_case(orc)

    def fresh(fn):
        c = dz.Context(0)
        try:
            return fn(c)
        finally:
            c.close()
    want = {form: fresh(lambda c: call(c, inp, fields, form)) for form in ("map_azim", "joint", "iso")}
    want_small = fresh(lambda c: small_call(c, small))
    assert len(want_small[2][2]) > 100
    for nwg in (0, 1):
        for form in ("map_azim", "joint", "iso"):
            assert same(call(ctx, inp, fields, form, rays_nwg=nwg), want[form]), (form, nwg)
        try:
            ctx.set_option("rays.nwg", nwg)
            assert same(small_call(ctx, small), want_small), nwg
        finally:
            ctx.set_option("rays.nwg", 0)
        assert same(call(ctx, inp, fields, "iso", rays_nwg=nwg), want["iso"]), nwg


def test_dense_twin_in_slots_that_serve_many_rays(ctx, batches):
    """rays.dense_twin: the rows go through the general loop, which reads the slot in both passes and in the twin's own emit pass"""
    inp, fields = batches["base"]

    def twin_call(nwg):
        try:
            ctx.set_option("rays.dense_twin", 1)
            ctx.set_option("rays.nwg", nwg)
            G, tpred, nb = bits.build(ctx, inp, fields, "joint")
        finally:
            ctx.set_option("rays.dense_twin", 0)
            ctx.set_option("rays.nwg", 0)
        Gd = G.take_twin()
        res = (np.array(tpred), nb, G.to_coo()), Gd.to_coo()
        G.free(); Gd.free()
        return res
    (g0, d0), (g1, d1) = twin_call(0), twin_call(1)
    assert same(g0, g1) and len(d0[2]) > len(g0[2][2]) and all(np.array_equal(a, b) for a, b in zip(d0, d1))
    assert same(g0, call(ctx, inp, fields, "joint"))


def test_keep_small_in_slots_that_serve_many_rays(ctx, batches):
    inp, fields = batches["base"]
    for form in ("iso", "map_azim"):
        free, capped = call(ctx, inp, fields, form, rays_keep_small=1), call(ctx, inp, fields, form, rays_keep_small=1, rays_nwg=1)
        assert same(free, capped) and len(free[2][2]) > len(call(ctx, inp, fields, form)[2][2]), form
