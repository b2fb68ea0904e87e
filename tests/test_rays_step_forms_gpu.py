"""-m gpu: the ray kernel's stepping loop by two routes.  By default it carries the start-point term of the scatter from one
sub-segment (and step) to the next, takes an interior form of the bilinear velocity and skips the refined-box work far from the
box; with option rays.plain_step = 1 it recomputes the start point in every step, always takes the general forms and always does
the refined-box work.  Both routes must give the same bits -- predicted times, boundary count, G triplets -- for iso, joint and map
rows, on tiled and column-major fields and with a 16-entry cell list (emit pass retraces), on three batches
(tests/rays_step_cases.py): the 17 x 15 batch of test_rays_gpu.py, one with every station in an edge cell (clipped rays, last row
and column) and one with the receivers inside their source's refined box.  The default route also stays within the oracle bars of
test_G_matches_oracle, and gives the bits the library gave before the loop was cut (tests/golden/rays_step_bits.json, recorded
by tools/rays_step_bits.py with the earlier library)."""
import json
import os
import sys

import numpy as np
import pytest

from tests import rays_step_cases as cases
from tests.bars import within
from tests.test_rays_gpu import G_FROB, G_MAX, TPRED_REL, dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rays_step_bits as bits   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(ctx, orc):
    """every ray call of this module, once: runs[name][(form, tiled, lcap16, plain)] = (tpred, n_boundary, triplets)"""
    out = {}
    for name in cases.NAMES:
        inp = bits.inputs(orc, name)
        res = {"inp": inp}
        for tiled in (False, True):
            fields = bits.fields_of(ctx, inp, keep=tiled)
            for form in bits.FORMS:
                for lcap16 in (False, True):
                    if lcap16 and (tiled or name != "base"):
                        continue
                    for plain in (0, 1):
                        try:
                            ctx.set_option("rays.plain_step", plain)
                            ctx.set_option("rays.lcap", 16 if lcap16 else 0)
                            G, tpred, nb = bits.build(ctx, inp, fields, form)
                        finally:
                            ctx.set_option("rays.plain_step", 0)
                            ctx.set_option("rays.lcap", 0)
                        assert ctx.stat("rays.tiled_fields") == float(tiled)
                        res[(form, tiled, lcap16, plain)] = (np.array(tpred), nb, G.to_coo())
                        G.free()
        out[name] = res
    return out


@pytest.mark.parametrize("name", cases.NAMES)
def test_plain_and_short_cut_steps_give_the_same_bits(runs, name):
    res = runs[name]
    keys = [k for k in res if k != "inp" and k[3] == 0]
    assert len(keys) == (12 if name == "base" else 8)
    for form, tiled, lcap16, _ in keys:
        (t0, nb0, coo0), (t1, nb1, coo1) = res[(form, tiled, lcap16, 0)], res[(form, tiled, lcap16, 1)]
        assert len(coo0[2]) > 100 and t0.min() > 0
        assert np.array_equal(t0, t1) and nb0 == nb1, (form, tiled, lcap16)
        assert all(np.array_equal(a, b) for a, b in zip(coo0, coo1)), (form, tiled, lcap16)
        # ... and neither the field layout nor the cell-list capacity moves a bit
        tr, nbr, coor = res[(form, False, False, 0)]
        assert np.array_equal(t0, tr) and nb0 == nbr and all(np.array_equal(a, b) for a, b in zip(coo0, coor)), (form, tiled, lcap16)


def test_the_batches_take_the_loop_through_its_forms(ctx, runs):
    """without these the comparisons above prove nothing: steps with one, two and three sub-segments, clipped rays, rays that end far
    from where they started (outside the refined box of their source, 8 coarse cells = 0.4 degrees around it) and rays inside it"""
    inp = runs["base"]["inp"]
    try:
        ctx.set_option("rays.keep_paths", 1)
        G, _, _ = bits.build(ctx, inp, bits.fields_of(ctx, inp), "iso")
        paths = ctx.ray_paths()
    finally:
        ctx.set_option("rays.keep_paths", 0)
    assert all(np.array_equal(a, b) for a, b in zip(G.to_coo(), runs["base"][("iso", False, False, 0)][2]))
    G.free()
    count = np.bincount(np.concatenate([cases.sub_segments(p) for p in paths if len(p) > 2]), minlength=4)
    print("steps with 1 / 2 / 3 sub-segments:", count[1:])
    assert count[1] > 100 and count[2] > 100 and count[3] >= 5
    reach = max(float(np.abs(p[0] - p[-1]).max()) for p in paths)
    assert reach > np.radians(1.0)                                       # far from the box: the refined-box work is skipped there
    assert runs["edge"][("iso", False, False, 0)][1] >= 10               # clipped rays
    assert runs["base"][("iso", False, False, 0)][1] == 0
    scx, scz, per, ray_f, rx, rz = runs["refined"]["inp"]["flat"]
    assert max(np.abs(rx - scx[ray_f]).max(), np.abs(rz - scz[ray_f]).max()) < np.radians(0.36)   # inside the box from the first step


@pytest.mark.parametrize("name", cases.NAMES)
def test_short_cut_steps_stay_within_the_oracle_bars(orc, runs, name):
    inp = runs[name]["inp"]
    rc, rw_o, ir_o, ic_o, ds_o, nb_o = orc.calsurfg(inp["vel"], cases.DEPZ, cases.GOXD, cases.GOZD, cases.DV, cases.DV, cases.T, cases.MINTHK,
                                                    *inp["tabs"], 4_000_000)
    assert rc == 0
    tpred, nb, (ir, ic, rw) = runs[name][("iso", False, False, 0)]
    assert len(tpred) == len(ds_o)
    m, n = len(ds_o), (cases.NX - 2) * (cases.NY - 2) * (len(cases.DEPZ) - 1)
    D, Do = dense(m, n, ir, ic, rw), dense(m, n, ir_o, ic_o, rw_o)
    print(name, "tpred rel", np.abs(tpred - ds_o).max() / np.abs(ds_o).max(), "G max |d|", np.abs(D - Do).max(),
          "G rel-Frobenius", np.linalg.norm(D - Do) / np.linalg.norm(Do))
    within("tpred rel", np.abs(tpred - ds_o).max() / np.abs(ds_o).max(), TPRED_REL)
    within("G max |d|", np.abs(D - Do).max(), G_MAX)
    within("G rel-Frobenius", np.linalg.norm(D - Do) / np.linalg.norm(Do), G_FROB)


def test_bits_of_the_library_before_the_cut(runs):
    golden = json.load(open(bits.GOLDEN))
    assert sorted(golden) == sorted(f"{n}.{f}" for n in cases.NAMES for f in bits.FORMS)
    for name in cases.NAMES:
        for form in bits.FORMS:
            tpred, nb, coo = runs[name][(form, False, False, 0)]
            want = golden[f"{name}.{form}"]
            assert (len(tpred), len(coo[2]), nb) == (want["m"], want["nnz"], want["n_boundary"]), (name, form)
            assert bits.sha1(coo, tpred) == want["sha1"], (name, form)
