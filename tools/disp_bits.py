"""A digest of every array that the entries built on surfdisp96 return, for a byte comparison of two builds of the library
(profiles/disp_once.md): dazim_dispersion_kernels, dazim_dispersion_kernels_typed, dazim_surfdisp96, dazim_ti_kernels and a short
dazim_mc_run on typed data.

    DAZIM_LIB=<one build> python tools/disp_bits.py --out a.txt
    DAZIM_LIB=<other build> python tools/disp_bits.py --out b.txt
    python tools/disp_bits.py --compare a.txt b.txt

One process per library; only the public Python API, so the file runs in another commit's tree as well.  The cases, on a 4 x 3 grid
of 5-knot columns and 6 periods unless stated:
  depthkernel   with and without depth kernels at three values of `sublayers`, one per division class of disp.hip's layer
                interpolation (RDEN, disp_pick_form), read off refineGrid2LayerMdl's fp32 arithmetic here on the CPU (den_class):
                  sublayers 3   2 nsub = 8 in every interval: powers of two              (RDEN 1)
                  sublayers 2   2 nsub = 6: on the list of verified fast divisions       (RDEN 2)
                  sublayers 16  2 nsub = 34: neither, the division stays                 (RDEN 0)
                and the power-of-two case with depth kernels again under each of the options disp.share = 0, disp.async = 2
                (device arrays; the curves' launch in teams as the plan decides, and with disp.team = 1 / 2: forced on / off),
                disp.ffwd = 0 and disp.pchunk = 4 (< 6 periods)
  typed         each of Rg, Lc, Lg alone, all four types in one call, and a curves-only call of the four types with 14 knots at
                sublayers 3 on 2 columns: the first plan with fewer than 64 items per workgroup (32; the line holds the statistic)
  surfdisp96    8 hand-built stacks of 6 layers, the first with a water layer, the last two with a low-velocity layer:
                iflsph {0, 1} x iwave {1, 2} x igr {0, 1} x mode {1, 2}
  ti_kernels    on the first case's model and curves
  mc.run        20 steps (10 burn-in, 10 recorded) with set_segments([Rc x 4, Lc x 4]) on the 5 x 5 set-up of
                tests/test_column_mc_gpu.disp_setup
One line per case and returned array: the first 16 hex digits of the SHA-256 of its bytes (counts by value).  --compare names every
line that differs and exits with 1 if there is one."""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

f32 = np.float32
DEPZ = np.array([0.0, 6.0, 15.0, 30.0, 55.0], f32)
PERIODS = np.array([5.0, 8.0, 12.0, 18.0, 26.0, 38.0])
RC, RG, LC, LG = (2, 0), (2, 1), (1, 0), (1, 1)
FASTDIV = (6, 10, 12, 14, 18, 20, 22, 24, 26, 28, 30, 36)   # disp_pick_form's list
SUBLAYERS = {3.0: "pow2", 2.0: "fastdiv", 16.0: "divide"}


def den_class(depz, sublayers):
    """the division class of a layer table: dz_refine_layers' nsub per interval in fp32, then disp_pick_form's rule"""
    cls = "pow2"
    for i in range(1, len(depz)):
        thk = f32(depz[i]) - f32(depz[i - 1])
        den = 2 * (int((thk + f32(1.0e-4)) / (thk / f32(sublayers))) + 1)
        if den & (den - 1):
            cls = "fastdiv" if den in FASTDIV and cls != "divide" else "divide"
    return cls


def columns(nz, ny, nx, depz):
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    vel = np.zeros((nz, ny, nx), f32)
    for k, z in enumerate(depz):
        vel[k] = 2.8 + 0.03 * z + 0.1 * np.sin(0.9 * ii + 0.5 * k) * np.cos(0.7 * jj)
    return vel


def stacks():
    """8 models x 6 layers: thk, vp, vs, rho"""
    vs = np.array([[0.0, 2.9, 3.2, 3.5, 3.9, 4.4], [2.6, 3.0, 3.3, 3.6, 4.0, 4.5], [3.0, 3.1, 3.3, 3.7, 4.1, 4.6],
                   [2.4, 2.9, 3.4, 3.8, 4.2, 4.7], [3.2, 3.3, 3.5, 3.6, 3.9, 4.3], [2.8, 3.2, 3.4, 3.9, 4.3, 4.4],
                   [3.1, 2.7, 3.4, 3.7, 4.0, 4.5], [2.9, 3.3, 3.0, 3.8, 4.2, 4.6]], f32)
    thk = np.array([[2.0, 4.0, 6.0, 10.0, 15.0, 0.0]] * 4 + [[3.0, 5.0, 8.0, 12.0, 20.0, 0.0]] * 4, f32)
    vp = f32(1.73) * vs
    rho = f32(0.32) * vp + f32(0.77)
    vp[0, 0], rho[0, 0] = 1.5, 1.03
    return thk, vp, vs, rho


def digest(v):
    if hasattr(v, "cpu"):
        v = v.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] if isinstance(v, np.ndarray) else repr(v)


def record(out):
    import dazimsurftomo_amd as dz
    from tests.test_column_mc_gpu import disp_setup
    ctx = dz.Context(0)

    def tables(case, pv, sen, nf):
        out.append(f"{case} pv {digest(pv)}")
        for name, a in zip(("sen_vs", "sen_vp", "sen_rho"), sen or ()):
            out.append(f"{case} {name} {digest(a)}")
        out.append(f"{case} n_failed {nf}")

    vel = columns(len(DEPZ), 3, 4, DEPZ)
    for sub, cls in SUBLAYERS.items():
        assert den_class(DEPZ, sub) == cls, (sub, den_class(DEPZ, sub))
        for kernels in (True, False):
            tables(f"depthkernel {cls} sublayers={sub:g} kernels={int(kernels)}", *ctx.depthkernel(vel, DEPZ, PERIODS, sub, kernels=kernels))
    default = {"disp.share": 1, "disp.ffwd": 1}
    for opts in ({"disp.share": 0}, {"disp.async": 2}, {"disp.async": 2, "disp.team": 1}, {"disp.async": 2, "disp.team": 2}, {"disp.ffwd": 0},
                 {"disp.pchunk": 4}):
        case = "depthkernel pow2 " + " ".join(f"{k}={v}" for k, v in opts.items())
        for k, v in opts.items():
            ctx.set_option(k, v)
        if "disp.async" in opts:   # (taken for device arrays only; the copies run on the auxiliary stream until sync)
            import torch
            pv, sen, nf = ctx.depthkernel(torch.from_numpy(vel).to("cuda:0"), DEPZ, PERIODS, 3.0)
            ctx.sync()
            out.append(f"{case} taken {ctx.stat('disp.async')!r} lanes per curve {ctx.stat_or('disp.team', 0)!r}")
        else:
            pv, sen, nf = ctx.depthkernel(vel, DEPZ, PERIODS, 3.0)
        tables(case, pv, sen, nf)
        for k in opts:
            ctx.set_option(k, default.get(k, 0))

    seg = lambda types: [(iw, ig, PERIODS) for iw, ig in types]
    for name, types in (("Rg", [RG]), ("Lc", [LC]), ("Lg", [LG]), ("Rc+Rg+Lc+Lg", [RC, RG, LC, LG])):
        tables(f"typed {name}", *ctx.dispersion_kernels_typed(vel, DEPZ, seg(types), 3.0))
    depz14 = np.cumsum(np.concatenate([[0.0], np.linspace(2.0, 5.0, 13)])).astype(f32)
    tables("typed curves-only 14 knots", *ctx.dispersion_kernels_typed(columns(14, 1, 2, depz14), depz14, seg([RC, RG, LC, LG]), 3.0, kernels=False))
    out.append(f"typed curves-only 14 knots items_per_wg {ctx.stat('disp_typed.items_per_wg')!r}")

    st = stacks()
    for iflsph, iwave, igr, mode in itertools.product((0, 1), (1, 2), (0, 1), (1, 2)):
        cg, nf = ctx.surfdisp96(*st, PERIODS, iflsph, iwave, mode, igr)
        out.append(f"surfdisp96 iflsph={iflsph} iwave={iwave} igr={igr} mode={mode} cg {digest(cg)}")
        out.append(f"surfdisp96 iflsph={iflsph} iwave={iwave} igr={igr} mode={mode} n_failed {nf}")

    pv, _, _ = ctx.depthkernel(vel, DEPZ, PERIODS, 3.0, kernels=False)
    out.append(f"ti_kernels lsen {digest(ctx.ti_kernels(vel, DEPZ, PERIODS, 3.0, pv))}")

    mc, truth, depz, periods = disp_setup(ctx, 5, 5, 0.01, 4)
    mc.set_segments([RC + (4,), LC + (4,)])
    out.append(f"mc.run no_root {mc.run(depz, 3.0, periods, 10, 10)}")
    for name, call in (("state", mc.state), ("result", mc.result)):
        for k, v in sorted(call().items()):
            out.append(f"mc.run {name}.{k} {digest(v)}")
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
    ap.add_argument("--out", default="disp_bits.txt")
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
