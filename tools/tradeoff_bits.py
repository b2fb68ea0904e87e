"""Every array the two trade-off sweeps return on the tests' problems, for a byte comparison of two builds of the library
(profiles/tradeoff_sweep_refactor.md; tools/posterior_bits.py does the same for the two posterior entries).

    DAZIM_LIB=<one build> python tools/tradeoff_bits.py --out a.npz
    DAZIM_LIB=<other build> python tools/tradeoff_bits.py --out b.npz
    python tools/tradeoff_bits.py --compare a.npz b.npz

One process per library.  The problems are those of tests/test_map_tradeoff_gpu.py and tests/test_model_tradeoff_gpu.py (CASES x REGS
with the sweep of their `case`), the long-row problems of tests/test_long_rows_gpu.py, and the period that cannot be factored, the
prior that is not positive definite and the period without data; the sweeps with dof and the evidence, without either, with x, and
with the option map_post.mfma at 1 and 0.  --compare names every array whose bytes differ (NaNs count by their bit pattern) and exits
with 1 if there is one."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP_KEYS = ("chi2", "reg2", "xnorm2", "logdet_a", "logdet_p", "dof", "gcv", "logev", "x", "n_failed", "mdata_p")


def keep(store, tag, out, keys):
    for k in keys:
        v = out.get(k)
        if v is None:
            continue
        if hasattr(v, "cpu"):
            v = v.cpu().numpy()
        store[f"{tag}/{k}"] = np.ascontiguousarray(v)


def sweeps(ctx, store, tag, call, scale, damp, tiles=(1, 0)):
    """the sweep with everything and x, without dof and the evidence, reversed without dof, its first point alone without the
    evidence; both tile forms"""
    for mfma in tiles:
        ctx.set_option("map_post.mfma", mfma)
        try:
            keep(store, f"{tag}/mfma{mfma}/full", call(scale, damp, x=True), SWEEP_KEYS)
            keep(store, f"{tag}/mfma{mfma}/bare", call(scale, damp, dof=False, evidence=False, x=False), SWEEP_KEYS)
            keep(store, f"{tag}/mfma{mfma}/nodof", call(scale[::-1].copy(), damp[::-1].copy(), dof=False, x=True), SWEEP_KEYS)
            keep(store, f"{tag}/mfma{mfma}/noev", call(scale[:1], damp[:1], evidence=False, x=False), SWEEP_KEYS)
        finally:
            ctx.set_option("map_post.mfma", 1)


def record(store):
    import dazimsurftomo_amd as dz
    from tests import map_posterior_ref as pref
    from tests import map_tradeoff_ref as ptref
    from tests import model_posterior_ref as mref
    from tests import model_tradeoff_ref as mtref
    from tests import test_map_tradeoff_gpu as mpt
    from tests import test_model_tradeoff_gpu as mt
    ctx = dz.Context(0)

    def maps(tag, prob, scale, damp, tiles=(1, 0)):
        A = mpt.matrix(ctx, prob)
        sweeps(ctx, store, tag, lambda s, d, **kw: mpt.call(ctx, A, prob, s, d, **kw), scale, damp, tiles)
        A.free()

    def model(tag, prob, scale, damp, tiles=(1, 0)):
        A = mt.matrix(ctx, prob)
        sweeps(ctx, store, tag, lambda s, d, **kw: mt.call(ctx, A, prob, s, d, **kw), scale, damp, tiles)
        A.free()

    for (shape, azim, kmax), cid in zip(mpt.CASES, mpt.CASE_IDS):
        for reg, rid in zip(pref.REGS, pref.REG_IDS):
            prob = ptref.problem(shape[0], shape[1], kmax, azim, reg)     # (the problem and sweep of mpt.case, without its reference)
            maps(f"map/{cid}/{rid}", prob, *ptref.sweep(prob))
    for (shape, joint), cid in zip(mt.CASES, mt.CASE_IDS):
        for reg, rid in zip(mref.REGS, mref.REG_IDS):
            prob = mtref.problem(shape, joint, reg)                       # (... of mt.case)
            model(f"model/{cid}/{rid}", prob, *mtref.sweep(prob))
    for mode in (False, True):
        prob = mtref.long_case(mode, mref.REGS[0])
        model(f"model/long-{int(mode)}", prob, *mtref.sweep(prob, (1.0,)))
        for through_dead in (False, True):
            prob = ptref.long_case(mode, pref.REGS[0], through_dead=through_dead)
            maps(f"map/long-{int(mode)}-dead{int(through_dead)}", prob, *ptref.sweep(prob, (1.0,)))
    ones, holes = np.ones((3, 3), np.float32), np.array([0.5, 0.0, 0.3], np.float32)
    semi = np.array([[1, 1, 1], [1, 0, 1], [2, 2, 2]], np.float32), np.array([0.3, 0.0, 0.3], np.float32)
    maps("map/unfactorable", ptref.problem(9, 5, 3, True, (0.8, 0.0), no_reg_period=1), ones, holes)
    maps("map/semidefinite", ptref.problem(3, 3, 3, True, (0.7, 0.3)), *semi)
    prob = ptref.without_data(ptref.problem(9, 5, 3, True, pref.REGS[0]), 1)
    scale, damp = ptref.sweep(prob)
    maps("map/no-data", prob, scale[:5], damp[:5])
    model("model/unfactorable", mtref.problem((9, 5, 3), True, (0.0, 0.5)), ones, holes)
    model("model/semidefinite", mtref.problem((3, 3, 2), True, (0.7, 0.3)), *semi)
    ctx.close()


def compare(a, b):
    x, y = np.load(a), np.load(b)
    names = sorted(set(x.files) | set(y.files))
    differ = []
    for k in names:
        if k not in x.files or k not in y.files:
            differ.append(f"{k}: only in {a if k in x.files else b}")
        elif x[k].dtype != y[k].dtype or x[k].shape != y[k].shape:
            differ.append(f"{k}: {x[k].dtype}{x[k].shape} against {y[k].dtype}{y[k].shape}")
        elif x[k].tobytes() != y[k].tobytes():
            u, v = x[k].reshape(-1).view(np.uint8), y[k].reshape(-1).view(np.uint8)
            differ.append(f"{k}: {int((u != v).reshape(-1, x[k].itemsize).any(axis=1).sum())} of {x[k].size} values differ")
    for line in differ:
        print(line)
    print(f"{len(names)} arrays, {len(differ)} differing")
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="tradeoff_bits.npz")
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
