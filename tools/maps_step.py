"""Map-mode vs iso-mode ray call on the same eikonal fields in one run (profiles/phase_maps.md).

    python tools/maps_step.py [--reps R] [--sources S] [--receivers N] [--workload s128|s256|s512]

The bench workload (default S-256: 16 periods x 1000 sources = 16 000 fields, 32 receivers each = 512 000 rays): dispersion tables
and fields once (the fields kept in the library, ttn = NULL), then R rounds of dazim_rays_build_G (iso mode, the model's depth
kernels) and dazim_rays_build_G_maps (azim 0, and azim 1 for information) on those fields.  Prints one JSON line with the kernel
seconds ("rays", HIP events on the context stream) and the host wall seconds of every call, their medians and the ratio
map / iso of the medians."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    import dazimsurftomo_amd as dz
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sources", type=int, default=1000)
    ap.add_argument("--receivers", type=int, default=32)
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="s256")
    a = ap.parse_args()
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
