"""Every array dazim_map_posterior and dazim_model_posterior return on the tests' problems, for a byte comparison of two builds of
the library (profiles/posterior_rows_refactor.md).

    DAZIM_LIB=<one build> python tools/posterior_bits.py --out a.npz
    DAZIM_LIB=<other build> python tools/posterior_bits.py --out b.npz
    python tools/posterior_bits.py --compare a.npz b.npz

One process per library.  The problems are CASES x REGS of tests/test_map_posterior_gpu.py (kmax 1 and 3) and of
tests/test_model_posterior_gpu.py, the long-row problems of tests/test_long_rows_gpu.py (the maps' with and without the rows through
the dead cell), and the period and the matrix that cannot be factored; each with sel and rows, and without sel, rows and the widths,
the model without depz too; all of it with the option map_post.mfma at 1 and 0.  `keep` and --compare are those of
tools/tradeoff_bits.py: every array whose bytes differ is named (NaNs count by their bit pattern), exit status 1 if there is one."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.tradeoff_bits import compare, keep  # noqa: E402


def record(store):
    import dazimsurftomo_amd as dz
    from tests import map_posterior_ref as pref
    from tests import model_posterior_ref as mref
    from tests import test_long_rows_gpu as lr
    from tests import test_map_posterior_gpu as mp
    from tests import test_model_posterior_gpu as mo
    ctx = dz.Context(0)

    def both_tiles(tag, calls):
        for mfma in (1, 0):
            ctx.set_option("map_post.mfma", mfma)
            try:
                for name, fn, keys in calls:
                    keep(store, f"{tag}/mfma{mfma}/{name}", fn(), keys + ("n_failed",))
            finally:
                ctx.set_option("map_post.mfma", 1)

    def maps(tag, prob, sel):
        A = mp.matrix(ctx, prob)
        both_tiles(tag, [("sel", lambda: mp.call(ctx, A, prob, sel), pref.OUTPUTS),
                         ("lean", lambda: mp.call(ctx, A, prob, None, width=False), pref.OUTPUTS)])
        A.free()

    def model(tag, prob, sel):
        A = mo.matrix(ctx, prob)
        both_tiles(tag, [("sel", lambda: mo.call(ctx, A, prob, sel), mref.OUTPUTS),
                         ("lean", lambda: mo.call(ctx, A, prob, None, width=False), mref.OUTPUTS),
                         ("nodepz", lambda: mo.call(ctx, A, prob, sel, depz=False), mref.OUTPUTS)])
        A.free()

    for (shape, azim), cid in zip(mp.CASES, mp.CASE_IDS):
        for reg, rid in zip(pref.REGS, pref.REG_IDS):
            for kmax in (1, 3):
                prob = mp.case(shape[0], shape[1], azim, reg, kmax)[0]
                maps(f"map/{cid}/{rid}/kmax{kmax}", prob, mp.some_sel(prob))
    for (shape, joint), cid in zip(mo.CASES, mo.CASE_IDS):
        for reg, rid in zip(mref.REGS, mref.REG_IDS):
            prob = mo.case(shape, joint, reg)[0]
            model(f"model/{cid}/{rid}", prob, mo.some_sel(prob["n"]))
    for mode in (False, True):
        for reg, rid in zip(mref.REGS, mref.REG_IDS):
            prob = mref.long_case(mode, reg)
            model(f"model/long-{int(mode)}/{rid}", prob, lr.model_sel(prob))
            for through_dead in (False, True):
                prob = pref.long_case(mode, reg, through_dead=through_dead)
                maps(f"map/long-{int(mode)}-dead{int(through_dead)}/{rid}", prob, lr.map_sel(prob))
    prob = mp.case(9, 5, True, (0.8, 0.0), 3, no_reg_period=1)[0]           # (period 1 cannot be factored)
    maps("map/unfactorable", prob, mp.some_sel(prob))
    prob = mref.problem(9, 5, 3, True, 0.0, 0.0, seed=1)                      # (the matrix cannot be factored)
    model("model/unfactorable", prob, mo.some_sel(prob["n"]))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="posterior_bits.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    store = {}
    record(store)
    np.savez(a.out, **store)
    print(f"{len(store)} arrays to {a.out} from {os.environ.get('DAZIM_LIB') or 'the built library'}")


if __name__ == "__main__":
    main()
