#!/usr/bin/env python
"""SHA-1 of G (rows, columns, values of its triplets) and of tpred for the batches of tests/rays_step_cases.py, iso, joint and map
rows: what tests/test_rays_step_forms_gpu.py compares with tests/golden/rays_step_bits.json.  The file was recorded with the
library built from the commit before the stepping loop's repeated arithmetic was cut; record it again only for a change that is
meant to move these bits.

    python tools/rays_step_bits.py                      print the hashes of the product library
    DAZIM_LIB=<other .so> python tools/rays_step_bits.py --write     record them in tests/golden/rays_step_bits.json"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "rays_step_bits.json")
FORMS = ("iso", "joint", "map", "map_azim")


def inputs(orc, name):
    """everything a ray call needs for batch `name`, dispersion inputs from the CPU oracle; joint rows with stand-in TI kernels"""
    from tests import rays_step_cases as cases
    from tests.test_rays_gpu import flatten
    vel, *tabs = cases.case(name)
    pv, sen = orc.depthkernel(vel, cases.DEPZ, cases.T, cases.MINTHK)
    lsen = (0.02 + 0.9 * np.random.default_rng(7).random((len(cases.DEPZ) - 1, cases.KMAX, cases.NX * cases.NY))).astype(np.float32)
    return dict(vel=vel, tabs=tabs, pv=pv, sen=sen, lsen=lsen, flat=flatten(*tabs))


def build(ctx, inp, fields, form):
    """(G, tpred, n_boundary) of one ray call"""
    from tests import rays_step_cases as c
    scx, scz, per, ray_f, rx, rz = inp["flat"]
    if form in ("iso", "joint"):
        return ctx.rays_build_G(c.NX, c.NY, c.GOXD, c.GOZD, c.DV, c.DV, inp["vel"], fields, scx, scz, per, ray_f, rx, rz, inp["sen"],
                                lsen=inp["lsen"] if form == "joint" else None)
    return ctx.rays_build_G_maps(c.NX, c.NY, c.GOXD, c.GOZD, c.DV, c.DV, fields, scx, scz, per, ray_f, rx, rz, azim=form == "map_azim")


def fields_of(ctx, inp, keep=False):
    from tests import rays_step_cases as c
    scx, scz, per = inp["flat"][:3]
    return ctx.fmm_batch(c.NX, c.NY, c.GOXD, c.GOZD, c.DV, c.DV, inp["pv"], scx, scz, per, keep_fields=keep)


def sha1(coo, tpred):
    h = hashlib.sha1()
    for a in (*coo, tpred):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    import dazimsurftomo_amd as dz
    from oracle.pyoracle import Oracle, build as build_oracle
    from tests import rays_step_cases as cases
    build_oracle()
    orc, ctx, out = Oracle(), dz.Context(0), {}
    for name in cases.NAMES:
        inp = inputs(orc, name)
        fields = fields_of(ctx, inp)
        for form in FORMS:
            G, tpred, nb = build(ctx, inp, fields, form)
            out[f"{name}.{form}"] = {"m": G.m, "nnz": G.nnz, "n_boundary": nb, "sha1": sha1(G.to_coo(), tpred)}
            G.free()
    ctx.close()
    print(json.dumps(out, indent=1))
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
