"""Golden vectors for tests/test_ti_cases_cpu.py and tests/test_ti_edges_gpu.py: what the flang build of the UNMODIFIED reference
depthkernelTI / tregn96 (oracle/_ref, `make -C oracle`) returns on the stress models of tests/ti_cases.py -- run in the build
container only; the .npz travels, the reference does not.

    python tests/golden/make_ti_stress_golden.py      ->  tests/golden/ti_stress.npz
"""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.pyoracle import Ref
from tests import ti_cases as K


def main():
    ref = Ref()
    out = {}
    for key, name, minthk in K.stress_runs():
        out[f"{key}_pv"], out[f"{key}_lsen"] = ref.depthkernel_ti(K.stress(name), K.DEPZ, K.T, minthk)
    np.savez_compressed(os.path.join(HERE, "ti_stress.npz"), **out)
    print(len(out), "arrays,", sum(a.nbytes for a in out.values()), "bytes")


if __name__ == "__main__":
    main()
