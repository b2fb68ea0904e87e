"""Golden vectors for tests/test_ref_geometries_cpu.py and tests/test_forward_geometries_gpu.py: what the flang build of the
UNMODIFIED reference routines (oracle/_ref, `make -C oracle`) returns on the grids of tests/geometry_cases.py -- unequal spacings,
66 and 72 N, the southern hemisphere, across the equator.  Run in the build container only; the .npz travels, the reference
does not.  Only arrays the reference's routines return are stored; the inputs are rebuilt from seeds by tests/geometry_cases.py.

    python tests/golden/make_ref_geometries_golden.py      ->  tests/golden/ref_geometries.npz

Per geometry and map (smooth, rough), the six sources along the first axis: ttn, nstsr (int16), box, gor, and for the other five
stations as receivers dsurf, fdm, rb.  veln and velnr are left out (they would take the file past the 1 MiB a committed file may
have; ttn depends on both).  On wide_lon also the five sources on the corner vertices and on a node (`edge`).  For wide_lon and north66 the
dense copies GVs (plain) and GVs, GGc, GGs (joint) of a 3-knot, 2-period batch.  The file is written with fixed zip time stamps,
so that a second run gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.pyoracle import Ref
from tests import geometry_cases as GC
from tests import synth

OUT = os.path.join(HERE, "ref_geometries.npz")


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


FIELD_KEYS = ("ttn", "nstsr", "box", "gor")
RAY_KEYS = ("dsurf", "fdm", "rb")


def stacked(out, tag, records, keys):
    """one array per key, the sources along the first axis"""
    for k in keys:
        a = np.stack([np.asarray(r[k]) for r in records])
        out[f"{tag}_{k}"] = a.astype(np.int16) if k == "nstsr" else a.astype(np.int32) if k == "rb" else a


def main():
    ref = Ref()
    out = {}
    nx, ny = GC.NX, GC.NY
    for name, geo in GC.GEOMETRIES.items():
        for rough in (False, True):
            pv, sx, sz = GC.field_inputs(geo, rough)
            recs = []
            for s in range(GC.NSRC):
                rcv = [j for j in range(GC.NSRC) if j != s]
                recs.append(ref.fmm_field(nx, ny, *geo, pv[0], sx[s], sz[s], sx[rcv], sz[rcv]))
            stacked(out, GC.tag(name, rough), recs, FIELD_KEYS + RAY_KEYS)
    geo = GC.GEOMETRIES["wide_lon"]
    pv, _, _ = GC.field_inputs(geo, False)
    ex, ez = synth.radians(*GC.corner_and_node_sources(nx, ny, geo))
    stacked(out, "wide_lon_edge", [ref.fmm_field(nx, ny, *geo, pv[0], ex[s], ez[s]) for s in range(len(ex))], FIELD_KEYS)
    for name in GC.DENSE_NAMES:
        geo = GC.GEOMETRIES[name]
        vel, *lists = GC.dense_case(geo)
        for joint in (False, True):
            dense = ref.calsurfg_dense(vel, GC.DENSE_DEPZ, *geo, GC.DENSE_T, GC.RAY_MINTHK, *lists, 400000, joint=joint)
            for i, d in enumerate(dense):
                out[f"{name}_dense_{int(joint)}_{i}"] = d
    # the reference's own Lsen_Gsc of that batch (the model does not depend on the geometry): the oracle's tregn96 is an independent
    # restatement that agrees to one ulp, so the joint rows are compared with these kernels fed to the oracle's row routine
    out["dense_lsen"] = ref.depthkernel_ti(vel, GC.DENSE_DEPZ, GC.DENSE_T, GC.RAY_MINTHK)[1]
    save_npz(OUT, out)
    print(len(out), "arrays,", sum(np.asarray(a).nbytes for a in out.values()), "bytes ->", os.path.getsize(OUT), "bytes in the file")


if __name__ == "__main__":
    main()
