#!/usr/bin/env python
"""Static instruction counts of the ray kernel's stepping loop, phase by phase.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S -DDZ_RAYS_MARK -Iinclude \
          -o /tmp/rays_mark.s dazimsurftomo_amd/csrc/rays.hip
    python tools/rays_phase_count.py /tmp/rays_mark.s [kernel-substring] [--blocks]

The DZ_RAYS_MARK build puts `; MARK n` comments into the step loop of rays_kernel: 0 = loop top, 1 = new point known, 2 = refined-box
work and cell indices done, 3 = source distance and stop test done, 4 = clipped, 5 = corner loads issued (path points, azimuth),
6 = crossings sorted, 7 = start-point block passed (rare), 8 = end point of a sub-segment evaluated (vel_at, basis), 9 = block change
passed (flush + reload, rare), 10 = scatter done and sub-segment loop left, 11 = step closed.  The markers are compiler barriers for
memory operations, so the marked build schedules its loads a little differently from the product; the counts of arithmetic are the
product's.  Blocks are taken in layout order: a wave-uniform rare block counts where the compiler put it (--blocks lists them).

Per region: VALU by issue class as in tools/fmm_phase_count.py (v2 / v4 / v8), of which fp64-class (conversions to and from double
and double arithmetic: the divr() quotients), the IEEE fp32 division sequence (v_div_scale / v_div_fmas / v_div_fixup / v_rcp), spill
traffic (scratch_* and v_readlane / v_writelane), scalar, LDS and global-memory instructions."""
import re
import sys
from collections import Counter

from fmm_phase_count import klass

NAMES = {(0, 1): "gradient and new point", (1, 2): "refined-box work, cell indices", (2, 3): "source distance, stop test",
         (3, 4): "clipping", (4, 5): "corner loads (path points, azimuth)", (5, 6): "crossing logic",
         (6, 7): "start-point block (rare)", (7, 8): "sub-segment: point, vel_at, basis", (8, 9): "sub-segment: block change (flush, rare)",
         (9, 10): "sub-segment: scatter, loop back", (10, 11): "step closed", (11, 0): "loop back", (9, 8): "(sub-segment loop back)",
         (10, 8): "(sub-segment loop back)"}


def extra(op):
    c = Counter()
    if op.startswith("v_") and ("f64" in op):
        c["f64"] += 1
    if op.startswith(("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_rcp_f32")):
        c["div"] += 1
    if op.startswith("v_div_fixup_f32"):
        c["ndiv"] += 1
    if op.startswith("scratch_"):
        c["scr"] += 1
    if op.startswith(("v_readlane", "v_writelane")):
        c["lane"] += 1
    if op.startswith("global_load"):
        c["gld"] += 1
    return c


def main(path, want, show_blocks):
    lines = open(path).read().split("\n")
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\S*rays_kernel\S*:", l) and want in l), None)
    if start is None:
        raise SystemExit("kernel not found: " + want)
    end = next(i for i in range(start + 100, len(lines)) if "s_endpgm" in lines[i])
    regions, cur, blocks = [], None, [["entry", Counter()]]
    for l in lines[start + 1:end + 1]:
        t = l.strip()
        m = re.match(r"; MARK (\d+)", t)
        if m:
            regions.append((cur, int(m.group(1)), blocks))
            cur, blocks = int(m.group(1)), [["(cont)", Counter()]]
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            blocks.append([m.group(1), Counter()])
            continue
        if not t or t.startswith((";", ".", "//")):
            continue
        op = t.split()[0]
        blocks[-1][1][klass(op, t.split(";")[0])] += 1
        blocks[-1][1].update(extra(op))
    regions.append((cur, None, blocks))
    head = "| phase | v2 | v4 | v8 | VALU | fp64-class | div. seq. (divisions) | scratch | lane r/w | s | lds | global loads | vm |"
    print(head + "\n|---|" + "---:|" * (head.count("|") - 2))
    row = lambda name, c: (f"| {name} | {c['v2']} | {c['v4']} | {c['v8']} | {c['v2'] + c['v4'] + c['v8']} | {c['f64']} | {c['div']} ({c['ndiv']}) | "
                           f"{c['scr']} | {c['lane']} | {c['s']} | {c['lds']} | {c['gld']} | {c['vm']} |")
    total, sub = Counter(), Counter()
    for a, b, blks in regions:
        if a is None or b is None:
            continue
        tot = Counter()
        for _, c in blks:
            tot.update(c)
        total.update(tot)
        if a in (7, 8, 9) :
            sub.update(tot)
        print(row(f"{a}->{b} {NAMES.get((a, b), '')}", tot))
        if show_blocks:
            for lab, c in blks:
                if sum(c.values()):
                    print(row(f"  `{lab}`", c))
    print(row("**sub-segment loop (7->10)**", sub))
    print(row("**step loop (0->11), rare blocks included**", total))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0], args[1] if len(args) > 1 else "rays_kernelILb0ELb0ELb1ELb0E", "--blocks" in sys.argv)
