"""Golden vectors for tests/test_disp_cases_cpu.py and tests/test_disp_edges_gpu.py: what the flang build of the UNMODIFIED reference
depthkernel / surfdisp96 (oracle/_ref, `make -C oracle ref`) returns on the stress runs of tests/disp_cases.py (models A and B at
minthk 0.5, 1 and 3, and both at 0.2 .. 1 s) -- run in the build container only; the .npz travels, the reference does not.

    python tests/golden/make_disp_stress_golden.py      ->  tests/golden/disp_stress.npz
"""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.pyoracle import Ref
from tests import disp_cases as D


def main():
    ref = Ref()
    cases = D.cases()
    out = {}
    for key in D.GOLDEN_KEYS:
        c = cases[key]
        pv, sen = ref.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"])
        out[f"{key}_pv"] = pv
        for name, s in zip(("vs", "vp", "rho"), sen):
            out[f"{key}_sen_{name}"] = s
    np.savez_compressed(D.GOLD, **out)
    print(len(out), "arrays,", sum(a.nbytes for a in out.values()), "bytes,", os.path.getsize(D.GOLD), "in the file")


if __name__ == "__main__":
    main()
