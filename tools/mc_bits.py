"""A digest of every array the Monte-Carlo sampler returns over its modes, for a byte comparison of two builds of the library
(profiles/mc_noise_once.md).

    DAZIM_LIB=<one build> python tools/mc_bits.py --out a.txt
    DAZIM_LIB=<other build> python tools/mc_bits.py --out b.txt
    python tools/mc_bits.py --compare a.txt b.txt

One process per library; only the public Python API, so the file runs in another commit's tree as well.  The grid: noise {off,
set_noise, one group, two groups, four groups} x prior {off, on} x proposal kind {0, 1} x {untempered, 4 rungs}, each a dazim_mc_run
of 60 burn-in steps (adaptation every 50: kind 1 factors once) and 20 recorded ones on the 5 x 5 model of
tests/test_column_mc_gpu.disp_setup.  One line per case and field: the SHA-256 of the bytes of state, result, cov_state,
temper_state, noise_state / noise_result, noise_groups_state / noise_groups_result and prior_state (scalars as their repr).
--compare names every line that differs and exits with 1 if there is one."""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"one": (np.zeros(8, int), [2.0], [1.0]), "two": (np.arange(8) % 2, [2.0, 1.5], [1.0, 0.5]),
          "four": (np.arange(8) // 2, [0.5, 0.25, 0.75, 1.0], [0.5, 1.0, 0.75, 2.0])}


def record(out):
    import dazimsurftomo_amd as dz
    from tests.test_column_mc_gpu import disp_setup
    ctx = dz.Context(0)
    for noise, prior, kind, ntemp in itertools.product(("off", "set_noise", "one", "two", "four"), (0, 1), (0, 1), (1, 4)):
        mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, 4)
        if kind:
            mc.set_proposal(1)
        if noise == "set_noise":
            mc.set_noise(2.0, 1.0)
        elif noise != "off":
            mc.set_noise_groups(*GROUPS[noise])
        if prior:
            mc.set_prior(3.0, 4.0)
        if ntemp > 1:
            mc.set_tempering(ntemp, 16.0, 1)
        mc.run(depz, 3.0, periods, 60, 20)
        calls = [("state", mc.state), ("result", mc.result), ("cov_state", mc.cov_state), ("temper_state", mc.temper_state),
                 ("noise_state", mc.noise_state), ("noise_groups_state", mc.noise_groups_state), ("prior_state", mc.prior_state)]
        if "nsum" in mc.noise_state():
            calls.append(("noise_result", mc.noise_result))
        if mc.noise_groups_state()["ngroup"]:
            calls.append(("noise_groups_result", mc.noise_groups_result))
        for name, call in calls:
            for k, v in sorted(call().items()):
                d = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] if isinstance(v, np.ndarray) else repr(v)
                out.append(f"noise={noise} prior={prior} kind={kind} ntemp={ntemp} {name}.{k} {d}")
        out.append(f"noise={noise} prior={prior} kind={kind} ntemp={ntemp} stat.mc.noise {ctx.stat('mc.noise')!r} "
                   f"stat.mc.noise_groups {ctx.stat('mc.noise_groups')!r}")
        mc.free()
    ctx.close()


def compare(a, b):
    x, y = open(a).read().splitlines(), open(b).read().splitlines()
    differ = [f"{p}\n    against {q}" for p, q in itertools.zip_longest(x, y, fillvalue="(missing)") if p != q]
    for line in differ:
        print(line)
    print(f"{max(len(x), len(y))} lines, {len(differ)} differing")
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="mc_bits.txt")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    out = []
    record(out)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"{len(out)} lines to {a.out} from {os.environ.get('DAZIM_LIB') or 'the built library'}")


if __name__ == "__main__":
    main()
