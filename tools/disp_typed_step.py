"""Times of the typed dispersion tables (dazim_dispersion_kernels_typed, DESIGN.md section 17, profiles/disp_typed.md).

    python tools/disp_typed_step.py [--reps R] [--grids test4,s256]

On the bundled test4_Yunnan columns (38 x 42 x 18 knots, sublayers 4, its 36 periods per segment) and on bench.py's S-256 model grid
(54 x 54 columns, 12 knots, sublayers 3, 16 periods), every array on the device:
  * the tuned Rayleigh-phase kernel (dazim_dispersion_kernels, kernel seconds "disp");
  * each other wave type as a one-segment typed call, and the three of them as one call -- (segment, column, variant) as the unit
    of work of ONE launch against three launches one after the other (kernel seconds "disp_typed", wall seconds of the call);
  * dazim_surfdisp96 fed the identical 1 + 6 nz layer stacks per column, built on the host as depthkernel builds them -- kernel
    seconds "surfdisp96", wall seconds of the call with its host prologue and its copies -- and, for a Love type, also fed only the
    1 + 4 nz models that the typed call runs (no Vp copies): the kernel-to-kernel ratio on the same models.
Prints one JSON line per grid with the medians of R rounds after a warm-up."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

f32 = np.float32
TYPES = {"Rg": (2, 1), "Lc": (1, 0), "Lg": (1, 1)}


def brocher(vs):
    """inv/CalSurfG.f90:49-53 in fp32"""
    v2 = vs * vs
    v3 = v2 * vs
    v4 = v3 * vs
    p = f32(0.9409) + f32(2.0947) * vs - f32(0.8206) * v2 + f32(0.2683) * v3 - f32(0.0251) * v4
    p2 = p * p
    p3 = p2 * p
    p4 = p3 * p
    p5 = p4 * p
    return p, f32(1.6612) * p - f32(0.4721) * p2 + f32(0.0671) * p3 - f32(0.0043) * p4 + f32(0.000106) * p5


def stacks(vel, depz, sublayers):
    """the 1 + 6 nz refined layer stacks of every column (refineGrid2LayerMdl, inv/CalSurfG.f90:2339-2365, fp32, vectorised over the
    models): thk, vp, vs, rho [ncol * (1 + 6 nz)][nlayer]"""
    nz = vel.shape[0]
    vs = np.ascontiguousarray(vel, f32).reshape(nz, -1).T                   # [ncol][nz]
    vp, rho = brocher(vs)
    kn = np.stack([vs, vp, rho], axis=1)                                     # [ncol][3][nz]
    var = np.repeat(kn[:, None], 1 + 6 * nz, axis=1)                         # [ncol][nvar][3][nz]
    half = f32(0.5) * f32(0.01)
    for i in range(nz):
        for q in range(3):
            b0 = kn[:, q, i]
            var[:, 1 + 6 * i + 2 * q, q, i] = b0 - half * b0
            var[:, 2 + 6 * i + 2 * q, q, i] = b0 + half * b0
    var = var.reshape(-1, 3, nz)
    depz = np.asarray(depz, f32)
    cols = [[] for _ in range(4)]
    for i in range(nz - 1):
        thk = depz[i + 1] - depz[i]
        nsub = int((thk + f32(1.0e-4)) / (thk / f32(sublayers))) + 1
        for j in range(1, nsub + 1):
            fm, den = f32(2 * j - 1), f32(2 * nsub)
            cols[0].append(np.full(len(var), thk / f32(nsub), f32))
            for a, q in ((1, 1), (2, 0), (3, 2)):
                cols[a].append(var[:, q, i] + fm * (var[:, q, i + 1] - var[:, q, i]) / den)
    cols[0].append(np.zeros(len(var), f32))
    for a, q in ((1, 1), (2, 0), (3, 2)):
        cols[a].append(var[:, q, nz - 1])
    return [np.ascontiguousarray(np.stack(c, axis=1)) for c in cols]


def one_grid(ctx, name, vel_h, depz, periods, sublayers, reps):
    import torch
    vel = torch.from_numpy(np.ascontiguousarray(vel_h, f32)).to("cuda:0")
    nz, ny, nx = vel_h.shape
    periods = np.asarray(periods, np.float64)
    med = lambda v: float(np.median(v))
    out = {"grid": f"{name}: {nx} x {ny} columns, {nz} knots, sublayers {sublayers:g}, {len(periods)} periods per segment", "reps": reps}

    def timed(fn, stat):
        ks, ws = [], []
        for rep in range(reps + 1):   # (round 0: warm-up -- code objects, scratch buffers)
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            w = time.perf_counter() - t0
            if rep:
                ks.append(ctx.kernel_seconds(stat))
                ws.append(w)
        return {"kernel_s": med(ks), "wall_s": med(ws)}

    out["Rc_tuned"] = timed(lambda: ctx.depthkernel(vel, depz, periods, sublayers), "disp")
    for k, (iw, ig) in TYPES.items():
        out[k + "_typed"] = timed(lambda: ctx.dispersion_kernels_typed(vel, depz, [(iw, ig, periods)], sublayers), "disp_typed")
    out["Rg+Lc+Lg_typed_one_call"] = timed(lambda: ctx.dispersion_kernels_typed(vel, depz, [(iw, ig, periods) for iw, ig in TYPES.values()], sublayers),
                                           "disp_typed")
    out["Rg+Lc+Lg_typed_three_calls_kernel_s"] = sum(out[k + "_typed"]["kernel_s"] for k in TYPES)
    out["items_per_workgroup"] = ctx.stat("disp_typed.items_per_wg")
    st = stacks(vel_h, depz, sublayers)
    v = np.arange(len(st[0])) % (1 + 6 * nz)
    no_vp = (v == 0) | (((v - 1) % 6) // 2 != 1)
    st_love = [np.ascontiguousarray(a[no_vp]) for a in st]
    out["surfdisp96_models"] = {"rayleigh": int(len(st[0])), "love": int(len(st_love[0]))}
    for k, (iw, ig) in TYPES.items():
        out[k + "_surfdisp96"] = same = timed(lambda: ctx.surfdisp96(*st, periods, 1, iw, 1, ig), "surfdisp96")
        if iw == 1:
            out[k + "_surfdisp96_without_vp_copies"] = same = timed(lambda: ctx.surfdisp96(*st_love, periods, 1, iw, 1, ig), "surfdisp96")
        out[k + "_typed_over_surfdisp96_kernel"] = out[k + "_typed"]["kernel_s"] / out[k + "_surfdisp96"]["kernel_s"]
        out[k + "_typed_over_surfdisp96_kernel_same_models"] = out[k + "_typed"]["kernel_s"] / same["kernel_s"]
    return out


def main():
    import dazimsurftomo_amd as dz
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grids", default="test4,s256")
    a = ap.parse_args()
    ctx = dz.Context(0)
    for g in a.grids.split(","):
        if g == "test4":
            d = np.load(os.path.join(ROOT, "tests", "golden", "test4_yunnan.npz"))
            res = one_grid(ctx, "test4_Yunnan", d["vel"], d["depz"], d["t"], float(d["minthk"]), a.reps)
        else:
            import bench
            res = one_grid(ctx, "S-256", bench.s256_model(), bench.DEPZ, bench.PERIODS, bench.MINTHK, a.reps)
        print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
