"""Times of the second step of the two-step method (profiles/depth_from_maps.md).

    python tools/depth_step.py [--reps R] [--big N] [--radial]

On bench.py's S-256 model grid (54 x 54 columns, 12 knots, 16 periods) and on an N x N grid of the same model (default 202: 200 x 200
inner cells), every array on the device, R rounds of: the dispersion call with kernels (kernel seconds "disp"; "disp.copies" too
where the perturbed copies ran on the auxiliary stream), dazim_vs_kernels ("vs_kernels"), dazim_column_lsq with the fp64 table and
one right-hand side and with the fp32 Lsen_Gsc table and two ("column_lsq"), and dazim_column_resolution beside each solve, on the
same table with the same weights and regularisers, without and with the rows ("column_resolution").  Kernel seconds are
dazim_last_kernel_seconds (HIP events on the context stream).  Prints one JSON line per grid with the medians and the ratio solve /
dispersion, then one line for the solve and the resolution call at nlay 31, 32, 33 and 63 on random tables (16 periods, the big
grid): an even nlay is where the lanes' reads along the rows of the [nlay][nlay] matrix meet in the same LDS banks
(profiles/depth_resolution.md).
--radial: instead, on the same two grids, an iteration of the radial-anisotropy mode with the 16 periods as
Rayleigh phase periods of the model (Vsv) and again as Love phase periods of the model times 1.03 (Vsh): the two typed dispersion
calls ("disp" + "disp.copies" for the Rayleigh segment, "disp_typed" for the Love segment), dazim_column_lsq_radial ("column_lsq_radial"), dazim_column_resolution_radial without the rows
("column_resolution_radial"), and beside them the two dazim_column_lsq calls on the same two tables, which is what couple = 0
computes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_grid(ctx, n, reps):
    import torch
    import bench
    bench.NX = bench.NY = n
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vel = T(bench.s256_model())
    nz, kmax, nlay = len(bench.DEPZ), len(bench.PERIODS), len(bench.DEPZ) - 1
    ncell = (n - 2) * (n - 2)
    rng = np.random.default_rng(1)
    r1 = T(0.05 * rng.standard_normal((1, kmax, n - 2, n - 2)).astype(np.float32))
    r2 = T(0.01 * rng.standard_normal((2, kmax, n - 2, n - 2)).astype(np.float32))
    w = T(np.full((kmax, n - 2, n - 2), 100.0, np.float32))
    pv, sen, _ = ctx.depthkernel(vel, bench.DEPZ, bench.PERIODS, bench.MINTHK)
    lsen = ctx.ti_kernels(vel, bench.DEPZ, bench.PERIODS, bench.MINTHK, pv)
    skern = ctx.vs_kernels(vel, sen)
    x1 = torch.empty((1, nlay, n - 2, n - 2), dtype=torch.float32, device=dev)
    x2 = torch.empty((2, nlay, n - 2, n - 2), dtype=torch.float32, device=dev)
    depz = T(np.asarray(bench.DEPZ, np.float32)[:nlay])
    runs = {"disp_s": [], "disp_copies_s": [], "vs_kernels_s": [], "column_lsq_fp64_nrhs1_s": [], "column_lsq_fp32_nrhs2_s": [],
            "column_resolution_fp64_s": [], "column_resolution_fp64_rows_s": [], "column_resolution_fp32_s": []}
    for rep in range(reps + 1):   # (round 0: warm-up -- code objects, scratch buffers)
        ctx.depthkernel(vel, bench.DEPZ, bench.PERIODS, bench.MINTHK, pv=pv, sen=sen)
        ctx.sync()
        t = {"disp_s": ctx.kernel_seconds("disp"), "disp_copies_s": ctx.kernel_seconds("disp.copies")}
        ctx.vs_kernels(vel, sen, skern=skern)
        t["vs_kernels_s"] = ctx.kernel_seconds("vs_kernels")
        ctx.column_lsq(n, n, nlay, skern, r1, w, 2.0, 0.0, x=x1)
        t["column_lsq_fp64_nrhs1_s"] = ctx.kernel_seconds("column_lsq")
        ctx.column_lsq(n, n, nlay, lsen, r2, w, 2.0, 0.0, x=x2)
        t["column_lsq_fp32_nrhs2_s"] = ctx.kernel_seconds("column_lsq")
        res = ctx.column_resolution(n, n, nlay, skern, w, 2.0, 0.0, depz=depz)
        t["column_resolution_fp64_s"] = ctx.kernel_seconds("column_resolution")
        ctx.column_resolution(n, n, nlay, skern, w, 2.0, 0.0, depz=depz, rows=True)
        t["column_resolution_fp64_rows_s"] = ctx.kernel_seconds("column_resolution")
        ctx.column_resolution(n, n, nlay, lsen, w, 2.0, 0.0, depz=depz)
        t["column_resolution_fp32_s"] = ctx.kernel_seconds("column_resolution")
        if rep:
            for k, v in t.items():
                runs[k].append(v)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    disp = med["disp_s"] + max(med["disp_copies_s"], 0.0)
    assert torch.isfinite(x1).all() and torch.isfinite(x2).all() and torch.isfinite(res["std_post"]).all() and res["n_failed"] == 0
    return {"grid": f"{n}x{n} columns ({ncell} inner cells), {nz} knots, {kmax} periods", "reps": reps, "median": med,
            "solve_fp64_over_disp": med["column_lsq_fp64_nrhs1_s"] / disp, "solve_fp32_over_disp": med["column_lsq_fp32_nrhs2_s"] / disp,
            "runs": runs}


def radial_grid(ctx, n, reps):
    import torch
    import bench
    bench.NX = bench.NY = n
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vsv = bench.s256_model()
    vsh = vsv.copy()
    vsh[:-1] *= np.float32(1.03)
    vsv, vsh = T(vsv), T(vsh)
    kmax, nlay = len(bench.PERIODS), len(bench.DEPZ) - 1
    rng = np.random.default_rng(1)
    rv, rh = (T(0.05 * rng.standard_normal((kmax, n - 2, n - 2)).astype(np.float32)) for _ in range(2))
    w = T(np.full((kmax, n - 2, n - 2), 100.0, np.float32))
    d0 = (vsh - vsv)[:nlay, 1:-1, 1:-1].contiguous()
    seg = {"v": [(2, 0, bench.PERIODS)], "h": [(1, 0, bench.PERIODS)]}
    runs = {"disp_typed_rayleigh_s": [], "disp_typed_love_s": [], "column_lsq_radial_s": [], "column_resolution_radial_s": [],
            "column_lsq_rayleigh_s": [], "column_lsq_love_s": []}
    for rep in range(reps + 1):   # (round 0: warm-up)
        t, kern = {}, {}
        for key, vel, name in (("v", vsv, "rayleigh"), ("h", vsh, "love")):
            pv, sen, nf = ctx.dispersion_kernels_typed(vel, bench.DEPZ, seg[key], bench.MINTHK)
            ctx.sync()
            # (a Rayleigh-phase segment is a dazim_dispersion_kernels call: its seconds are under "disp" and "disp.copies")
            t[f"disp_typed_{name}_s"] = (ctx.kernel_seconds("disp") + max(ctx.kernel_seconds("disp.copies"), 0.0) if key == "v"
                                         else ctx.kernel_seconds("disp_typed"))
            kern[key] = ctx.vs_kernels(vel, sen)
            assert nf == 0
        x, ne, _ = ctx.column_lsq_radial(n, n, nlay, kern["v"], kern["h"], rv, rh, w, w, d0, 2.0, 0.0, 5.0)
        t["column_lsq_radial_s"] = ctx.kernel_seconds("column_lsq_radial")
        res = ctx.column_resolution_radial(n, n, nlay, kern["v"], kern["h"], w, w, 2.0, 0.0, 5.0)
        t["column_resolution_radial_s"] = ctx.kernel_seconds("column_resolution_radial")
        ctx.column_lsq(n, n, nlay, kern["v"], rv[None], w, 2.0, 0.0)
        t["column_lsq_rayleigh_s"] = ctx.kernel_seconds("column_lsq")
        ctx.column_lsq(n, n, nlay, kern["h"], rh[None], w, 2.0, 0.0)
        t["column_lsq_love_s"] = ctx.kernel_seconds("column_lsq")
        if rep:
            for k, v in t.items():
                runs[k].append(v)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    assert ne == 0 and torch.isfinite(x).all() and torch.isfinite(res["std"]).all() and res["n_failed"] == 0
    lds = 8 * (nlay * (2 * nlay + 1) + 2 * kmax * (nlay + 2) + 2 * nlay)
    return {"grid": f"{n}x{n} columns ({(n - 2) ** 2} inner cells), {nlay} knots per profile, {kmax} Rayleigh + {kmax} Love periods",
            "reps": reps, "lds_bytes_per_workgroup": lds, "median": med,
            "radial_over_two_column_lsq": med["column_lsq_radial_s"] / (med["column_lsq_rayleigh_s"] + med["column_lsq_love_s"]),
            "runs": runs}


def nlay_sweep(ctx, n, reps, kmax=16):
    """the solve and the resolution call at nlay 31, 32, 33 and 63, random fp64 tables: medians of `reps` rounds after a warm-up"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2)
    out = {}
    for nlay in (31, 32, 33, 63):
        kern = torch.from_numpy(rng.standard_normal((nlay, kmax, n * n))).to(dev)
        r = torch.from_numpy(rng.standard_normal((1, kmax, n - 2, n - 2)).astype(np.float32)).to(dev)
        depz = torch.arange(nlay, dtype=torch.float32, device=dev)
        x = torch.empty((1, nlay, n - 2, n - 2), dtype=torch.float32, device=dev)
        runs = {"column_lsq_s": [], "column_resolution_s": [], "column_resolution_rows_s": []}
        for i in range(reps + 1):
            ctx.column_lsq(n, n, nlay, kern, r, None, 0.7, 0.3, x=x)
            t = {"column_lsq_s": ctx.kernel_seconds("column_lsq")}
            ctx.column_resolution(n, n, nlay, kern, None, 0.7, 0.3, depz=depz)
            t["column_resolution_s"] = ctx.kernel_seconds("column_resolution")
            if nlay < 63:                              # (the rows of 40 000 cells at nlay 63 are 635 MB: left out)
                ctx.column_resolution(n, n, nlay, kern, None, 0.7, 0.3, depz=depz, rows=True)
                t["column_resolution_rows_s"] = ctx.kernel_seconds("column_resolution")
            if i:
                for k, v in t.items():
                    runs[k].append(v)
        out[f"nlay{nlay}"] = {k: float(np.median(v)) for k, v in runs.items() if v}
        del kern, r, x
    return {"sweep": f"{n}x{n} columns, {kmax} periods, random fp64 tables, smooth 0.7, damp 0.3", "reps": reps, "median": out}


def main():
    import dazimsurftomo_amd as dz
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=202)
    ap.add_argument("--radial", action="store_true")
    a = ap.parse_args()
    ctx = dz.Context(0)
    for n in (54, a.big):
        print(json.dumps((radial_grid if a.radial else one_grid)(ctx, n, a.reps)), flush=True)
    if not a.radial:
        print(json.dumps(nlay_sweep(ctx, a.big, a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
