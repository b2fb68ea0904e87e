"""Map-mode vs iso-mode ray call on the same eikonal fields in one run (profiles/phase_maps.md).

    python tools/maps_step.py [--reps R] [--sources S] [--receivers N] [--workload s128|s256|s512|test1] [--posterior]

The bench workload (default S-256: 16 periods x 1000 sources = 16 000 fields, 32 receivers each = 512 000 rays): dispersion tables
and fields once (the fields kept in the library, ttn = NULL), then R rounds of dazim_rays_build_G (iso mode, the model's depth
kernels) and dazim_rays_build_G_maps (azim 0, and azim 1 for information) on those fields.  Prints one JSON line with the kernel
seconds ("rays", HIP events on the context stream) and the host wall seconds of every call, their medians and the ratio
map / iso of the medians.

--posterior (profiles/map_posterior.md): instead of the ray A/B, per mode (iso, joint) one map iteration on those fields (map rows,
CalDdatSigma weights, 2-D regularisation, LSMR: host wall seconds) and R calls of dazim_map_posterior on that iteration's matrix with
either tile form (option map_post.mfma 0 / 1): the medians of its parts (stats map_post.gram, .factor, .inverse, .c, .rows) and of
the whole call.  --workload test1: the shape of the test1 example (17 x 17 vertices, periods 5 12 25 40 s; use --sources 10
--receivers 9)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


PARTS = ("map_post.gram", "map_post.factor", "map_post.inverse", "map_post.c", "map_post.rows", "map_posterior")


def posterior_leg(a, ctx, bench, fields, rays, d_tp):
    import torch
    NX, NY, kmax = bench.NX, bench.NY, len(bench.PERIODS)
    rng = np.random.default_rng(7)
    for mode in a.modes.split(","):
        azim = mode == "joint"
        w = np.array([2.0] * kmax + [2.0] * (2 * kmax if azim else 0), np.float32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G, tp, _ = ctx.rays_build_G_maps(NX, NY, bench.GOXD, bench.GOZD, bench.DV, bench.DV, fields, *rays, azim=azim, tpred=d_tp)
        tp = tp.cpu().numpy()
        tobs = (tp * (1.0 + 0.01 * rng.standard_normal(len(tp)))).astype(np.float32)
        m_data = G.m
        _, _, rhs, _ = ctx.weight_data(G, tobs, tp)
        G.append_laplacian2d(NX, NY, w)
        b = np.concatenate([rhs, np.zeros(G.m - m_data, np.float32)])
        _, info = ctx.lsmr(G, b, 0.01, 1e-5, 1e-4, 200, 500, 10)
        iteration_s = time.perf_counter() - t0
        out = {"workload": a.workload, "mode": mode, "rays": int(m_data), "n_g": (3 if azim else 1) * (NX - 2) * (NY - 2), "kmax": kmax,
               "nnz": int(G.nnz), "map_iteration_wall_s": iteration_s, "lsmr_itn": info["itn"], "reps": a.reps}
        for mfma in (0, 1):
            ctx.set_option("map_post.mfma", mfma)
            runs = []
            for r in range(a.reps + 1):                  # (the first call allocates the workspace: not counted)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = ctx.map_posterior(G, m_data, NX, NY, kmax, azim, 0.01)
                wall = time.perf_counter() - t0
                if r:
                    runs.append(dict({k: ctx.stat(k) for k in PARTS}, wall_s=wall))
            out[f"mfma{mfma}"] = {k: float(np.median([x[k] for x in runs])) for k in runs[0]}
            out[f"mfma{mfma}"]["median_std_post_c"] = float(np.median(res["std_post"][0]))
            out[f"mfma{mfma}"]["n_failed"] = res["n_failed"]
        ctx.set_option("map_post.mfma", 1)
        out["nb"] = ctx.stat("map_post.nb")
        print(json.dumps(out), flush=True)
        G.free()


def main():
    import torch
    import bench
    import dazimsurftomo_amd as dz
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sources", type=int, default=1000)
    ap.add_argument("--receivers", type=int, default=32)
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS) + ["test1"], default="s256")
    ap.add_argument("--posterior", action="store_true")
    ap.add_argument("--modes", default="iso,joint", help="--posterior: which of iso, joint")
    a = ap.parse_args()
    if a.workload == "test1":
        bench.NX = bench.NY = 17
        bench.PERIODS = np.array([5.0, 12.0, 25.0, 40.0])
    else:
        bench.set_workload(a.workload)
    NX, NY, G0, DV = bench.NX, bench.NY, (bench.GOXD, bench.GOZD), bench.DV
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ctx = dz.Context(0)
    kmax = len(bench.PERIODS)
    vel = bench.s256_model()
    scx, scz, per, fray, rcx, rcz = bench.workload(a.sources, a.receivers, 0)
    nfield, nray = len(scx), len(rcx)
    g = dz.geometry(NX, NY, G0[0], G0[1], DV, DV)
    d_vel, d_scx, d_scz, d_per, d_fray, d_rcx, d_rcz = (T(x) for x in (vel, scx, scz, per, fray, rcx, rcz))
    pv, sen, _ = ctx.depthkernel(d_vel, bench.DEPZ, bench.PERIODS, bench.MINTHK)
    bufs = dict(veln=torch.empty((kmax, g.nnx, g.nnz), dtype=torch.float32, device=dev),
                ttnr=torch.empty((nfield, 129, 129), dtype=torch.float32, device=dev),
                nstsr=torch.empty((nfield, 129, 129), dtype=torch.int32, device=dev),
                boxes=torch.empty((nfield, 12), dtype=torch.int32, device=dev),
                status=torch.empty((nfield,), dtype=torch.int32, device=dev))
    fields = ctx.fmm_batch(NX, NY, G0[0], G0[1], DV, DV, pv, d_scx, d_scz, d_per, keep_fields=True, **bufs)
    d_tp = torch.empty((nray,), dtype=torch.float32, device=dev)
    if a.posterior:
        posterior_leg(a, ctx, bench, fields, (d_scx, d_scz, d_per, d_fray, d_rcx, d_rcz), d_tp)
        ctx.close()
        return
    runs = {"iso": [], "map": [], "map_azim": []}
    nnz = {}

    def one(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "iso":
            G, _, _ = ctx.rays_build_G(NX, NY, G0[0], G0[1], DV, DV, d_vel, fields, d_scx, d_scz, d_per, d_fray, d_rcx, d_rcz, sen,
                                       tpred=d_tp)
        else:
            G, _, _ = ctx.rays_build_G_maps(NX, NY, G0[0], G0[1], DV, DV, fields, d_scx, d_scz, d_per, d_fray, d_rcx, d_rcz,
                                            azim=kind == "map_azim", tpred=d_tp)
        wall = time.perf_counter() - t0
        runs[kind].append({"rays_s": ctx.kernel_seconds("rays"), "wall_s": wall})
        nnz[kind] = G.nnz
        G.free()

    for kind in ("iso", "map", "map_azim"):   # warm-up: scratch buffers, code objects
        one(kind)
    for kind in runs:
        runs[kind].clear()
    for _ in range(a.reps):
        for kind in ("iso", "map", "map_azim"):
            one(kind)
    med = {k: {q: float(np.median([r[q] for r in v])) for q in ("rays_s", "wall_s")} for k, v in runs.items()}
    out = {"workload": a.workload, "fields": nfield, "rays": nray, "reps": a.reps, "nnz": nnz, "median": med,
           "map_over_iso_rays_s": med["map"]["rays_s"] / med["iso"]["rays_s"],
           "map_over_iso_wall_s": med["map"]["wall_s"] / med["iso"]["wall_s"], "runs": runs}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
