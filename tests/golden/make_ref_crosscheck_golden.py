"""Golden vectors for tests/test_ref_crosscheck.py and the random-model test of tests/test_surfdisp_full_cpu.py: what the flang
build of the UNMODIFIED reference routines (oracle/_ref, `make -C oracle`) returns on the seeded inputs those tests build --
run in the build container only; the .npz travels, the reference does not.  The tests compare the oracle with these bit for bit.

    python tests/golden/make_ref_crosscheck_golden.py      ->  tests/golden/ref_crosscheck.npz
"""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.pyoracle import Ref
from tests import test_ref_crosscheck as X
from tests import test_surfdisp_full_cpu as S


def main():
    ref = Ref()
    out = {}
    c = X.fields_case()
    for k, s in c["fields"]:
        r = ref.fmm_field(c["nx"], c["ny"], *c["box"], c["pv"][k], c["sx"][s], c["sz"][s])
        for name in X.FIELD_KEYS:
            out[f"fields_{k}_{s}_{name}"] = r[name]
    c = X.dispersion_case()
    out["disp_pv"], sen = ref.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"])
    for q in range(3):
        out[f"disp_sen_{q}"] = sen[q]
    c = X.lsmr_case()
    for ls in c["local_sizes"]:
        x, info = ref.lsmr(*c["system"], *c["cfg"], ls)
        out[f"lsmr_{ls}_x"], out[f"lsmr_{ls}_itn_istop"] = x, np.array([info["itn"], info["istop"]], np.int32)
    c = X.ti_test4_case()
    out["ti_test4_pv"], out["ti_test4_ls"] = ref.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    c = X.ti_random_case()
    for minthk in c["minthks"]:
        out[f"ti_random_{minthk:g}_pv"], out[f"ti_random_{minthk:g}_ls"] = ref.depthkernel_ti(c["vel"], c["depz"], c["t"], minthk)
    for joint in (False, True):
        c = X.dense_case()
        vel, *lists = c["case"]
        dense = ref.calsurfg_dense(vel, c["depz"], c["goxd"], c["gozd"], c["dv"], c["dv"], c["t"], c["minthk"], *lists, 400000, joint=joint)
        for i, d in enumerate(dense):
            out[f"dense_{int(joint)}_{i}"] = d
    for trial, (thk, vp, vs, rho) in enumerate(S.random_models()):
        for s, w, m, q in S.RANDOM_COMBOS:
            out[f"surfdisp_{trial}_{s}{w}{m}{q}"] = ref.surfdisp96_full(thk, vp, vs, rho, S.RANDOM_PERIODS, s, w, m, q)
    np.savez_compressed(os.path.join(HERE, "ref_crosscheck.npz"), **out)
    print(len(out), "arrays,", sum(a.nbytes for a in out.values()), "bytes")


if __name__ == "__main__":
    main()
