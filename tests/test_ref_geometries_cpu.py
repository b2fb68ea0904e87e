"""CPU (-m "not gpu"): the oracle against the unmodified reference on grids with unequal spacings and at other latitudes
(tests/geometry_cases.py), through tests/golden/ref_geometries.npz (tests/golden/make_ref_geometries_golden.py: the flang build
of the reference on the same seeded inputs).  Bit for bit, as tests/test_ref_crosscheck.py does on its one 9 x 14 grid at 28 N:
geometry and refined boxes, eikonal fields (nstsr, ttn; the gridder and bsplrefine through them), receiver times, ray paths /
Frechet weights, and the dense copies of a whole CalSurfG / CalSurfGAnisoJoint batch.

Premises asserted here: rc == 0 everywhere, no NaN in any recorded fdm, rb == 0 (no ray leaves through the grid's boundary).
"""
import os

import numpy as np
import pytest

from tests import geometry_cases as GC
from tests import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_geometries.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLD)


def check_field(orc, g, pv, veln, scx, scz, ref, tag, s):
    """one source's eikonal outputs against the record; returns what the ray routines need"""
    rc, ttn, ttnr, nstsr, velnr, box = orc.fmm_field(g, pv, veln, scx, scz)
    assert rc == 0
    assert [box.vnl, box.vnr, box.vnt, box.vnb, box.nnxr, box.nnzr, box.isx, box.isz] == list(ref[f"{tag}_box"][s])
    assert np.array_equal(np.array([box.goxr, box.gozr, box.dnxr, box.dnzr], np.float32), ref[f"{tag}_gor"][s])
    assert np.array_equal(nstsr, ref[f"{tag}_nstsr"][s].astype(np.int32)), (tag, s)
    assert np.array_equal(ttn, ref[f"{tag}_ttn"][s]), (tag, s, np.abs(ttn - ref[f"{tag}_ttn"][s]).max())
    return ttn, ttnr, nstsr, box


@pytest.mark.parametrize("rough", [False, True], ids=["smooth", "rough"])
@pytest.mark.parametrize("name", GC.NAMES)
def test_fields_and_rays(orc, ref, name, rough):
    geo = GC.GEOMETRIES[name]
    tag = GC.tag(name, rough)
    pv, sx, sz = GC.field_inputs(geo, rough)
    g = orc.geometry(GC.NX, GC.NY, *geo)
    veln = orc.gridder(g, pv[0])
    fdm_ref, rb_ref = ref[f"{tag}_fdm"], ref[f"{tag}_rb"]
    assert np.isfinite(fdm_ref).all() and not rb_ref.any()
    for s in range(GC.NSRC):
        ttn, ttnr, nstsr, box = check_field(orc, g, pv[0], veln, sx[s], sz[s], ref, tag, s)
        for i, r in enumerate(j for j in range(GC.NSRC) if j != s):
            e, t = orc.srtimes(g, veln, ttn, sx[s], sz[s], sx[r], sz[r])
            assert e == 0 and np.float32(t) == ref[f"{tag}_dsurf"][s][i], (tag, s, r)
            e, fdm, rb = orc.rpaths(g, box, veln, ttn, ttnr, nstsr, sx[s], sz[s], sx[r], sz[r])
            assert e == 0 and rb == 0 and np.array_equal(fdm, fdm_ref[s][i]), (tag, s, r)


def test_corner_and_node_sources_on_wide_lon(orc, ref):
    """sources exactly on the four corner vertices and on a node of the (0.25, 0.4) grid: the reference stays finite there"""
    geo = GC.GEOMETRIES["wide_lon"]
    pv, _, _ = GC.field_inputs(geo, False)
    ex, ez = synth.radians(*GC.corner_and_node_sources(GC.NX, GC.NY, geo))
    g = orc.geometry(GC.NX, GC.NY, *geo)
    veln = orc.gridder(g, pv[0])
    assert np.isfinite(ref["wide_lon_edge_ttn"]).all()
    for s in range(len(ex)):
        check_field(orc, g, pv[0], veln, ex[s], ez[s], ref, "wide_lon_edge", s)


@pytest.mark.parametrize("joint", [False, True], ids=["plain", "joint"])
@pytest.mark.parametrize("name", GC.DENSE_NAMES)
def test_dense_copies_of_a_whole_batch(orc, ref, name, joint):
    """GVs (GGc, GGs) as CalSurfG / CalSurfGAnisoJoint fill them for a 3-knot, 2-period batch -- the reference's own period, source
    and receiver loops, dispersion included -- against orc.dense_row per ray; and orc.calsurfg's triplets are that batch's rows"""
    from tests.test_rays_gpu import flatten
    geo = GC.GEOMETRIES[name]
    nx, ny, depz, t, minthk = GC.NX, GC.NY, GC.DENSE_DEPZ, GC.DENSE_T, GC.RAY_MINTHK
    vel, *lists = GC.dense_case(geo)
    dense = [ref[f"{name}_dense_{int(joint)}_{i}"] for i in range(3 if joint else 1)]
    assert all(np.isfinite(d).all() for d in dense)
    pv, sen = orc.depthkernel(vel, depz, t, minthk)
    lsen = None
    if joint:
        # Lsen_Gsc: the oracle's tregn96 is restated independently and agrees with the reference to one ulp (DESIGN.md section 2,
        # the 2e-7 of test_ref_crosscheck.py), whatever the grid: 6 of the 720 entries differ here, by 1.1e-7 of the maximum.  The
        # rows are therefore formed from the reference's own kernels, so that the ray part is held to the reference bit for bit.
        lsen = ref["dense_lsen"]
        own = orc.depthkernel_ti(vel, depz, t, minthk)[1]
        assert np.abs(own - lsen).max() <= 2e-7 * np.abs(lsen).max()
    scx, scz, per, ray_f, rx, rz = flatten(*lists)
    g = orc.geometry(nx, ny, *geo)
    npar = (nx - 2) * (ny - 2) * (len(depz) - 1)
    assert dense[0].shape == (len(rx), npar) and np.abs(dense[0]).max() > 0
    rows_rw, rows_ir, rows_ic = [], [], []
    for f in range(len(scx)):
        k = int(per[f]) - 1
        veln = orc.gridder(g, pv[k])
        rc, ttn, ttnr, nstsr, velnr, box = orc.fmm_field(g, pv[k], veln, scx[f], scz[f])
        assert rc == 0
        for r in np.nonzero(ray_f == f)[0]:
            if joint:
                rc, fdm, fdmc, fdms, rb = orc.rpaths_azim(g, box, veln, ttn, ttnr, nstsr, scx[f], scz[f], rx[r], rz[r])
                rows = orc.dense_row(vel, fdm, sen, k, fdmc, fdms, lsen)
            else:
                rc, fdm, rb = orc.rpaths(g, box, veln, ttn, ttnr, nstsr, scx[f], scz[f], rx[r], rz[r])
                rows = [orc.dense_row(vel, fdm, sen, k)]
                rw, ir, ic = orc.emit_row(vel, fdm, sen, k, r + 1)
                rows_rw.append(rw); rows_ir.append(ir); rows_ic.append(ic)
            assert rc == 0 and rb == 0
            for b, (got, want) in enumerate(zip(rows, dense)):
                assert np.array_equal(got, want[r]), (name, f, r, b, np.abs(got - want[r]).max())
    if not joint:   # the batch driver of the oracle walks the same loops: its triplets are the per-ray rows, in order
        rc, rw_o, ir_o, ic_o, ds_o, nb_o = orc.calsurfg(vel, depz, *geo, t, minthk, *lists, 400000)
        assert rc == 0 and nb_o == 0
        assert np.array_equal(rw_o, np.concatenate(rows_rw)) and np.array_equal(ir_o, np.concatenate(rows_ir))
        assert np.array_equal(ic_o, np.concatenate(rows_ic))
