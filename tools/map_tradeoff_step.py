"""Where dazim_map_tradeoff's time goes (profiles/map_tradeoff.md).

    python tools/map_tradeoff_step.py [--cases test4,s256] [--modes iso,azim] [--points 1,9] [--sources S] [--receivers N] [--posterior R]

Per case and mode one map iteration's matrix and weighted right-hand side as SurfPhaseMaps_amd builds them (the case's dispersion
curves as maps, eikonal fields, map rows, CalDdatSigma weights, 2-D regularisation with the case's weights; tools/model_post_step.py's
cases: test4 = 38 x 42 vertices, 36 periods; s256 = the bench workload, 54 x 54 vertices, 16 periods), then dazim_map_tradeoff with the
program's factors 10^(-1 + 2k/(K-1)) on every block and the case's damping, for each K of --points (K = 1: the factor 1 alone), with
dof and the evidence, and for the largest K once more without either.  Per call the stats map_trade.gram (once per period: it must not
grow with K), .factor, .solve, .inverse, map_tradeoff and map_trade.grams, the host wall seconds, and the picks of the totals.  One
JSON line per call.  --posterior R: instead of the sweeps, R + 1 calls of dazim_map_posterior on that matrix (the first allocates the
workspace and is not counted) and the medians of its stats map_post.gram, .factor, .inverse, .c, .rows and map_posterior and of the
host wall seconds (profiles/posterior_rows_refactor.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.model_post_step import example, golden_inputs, s256   # noqa: E402
from tools.model_tradeoff_step import factors                     # noqa: E402

POST_PARTS = ("map_post.gram", "map_post.factor", "map_post.inverse", "map_post.c", "map_post.rows", "map_posterior")
PARTS = ("map_trade.gram", "map_trade.factor", "map_trade.solve", "map_trade.inverse", "map_tradeoff", "map_trade.grams")


def one_case(ctx, name, c, azim, points, posterior=0):
    import torch
    nx, ny, kmax = c["nx"], c["ny"], len(c["periods"])
    geo = (nx, ny, c["goxd"], c["gozd"], c["dvxd"], c["dvzd"])
    scx, scz, per, ray_f, rx, rz = c["survey"]
    pv, _, _ = ctx.depthkernel(c["vel"], c["depz"], c["periods"], c["minthk"], kernels=False)
    fields = ctx.fmm_batch(*geo, pv, scx, scz, per)
    G, tp, _ = ctx.rays_build_G_maps(*geo, fields, scx, scz, per, ray_f, rx, rz, azim=azim)
    del fields
    m_data = G.m
    tp = np.asarray(tp).copy()
    tobs = (tp * (1.0 + 0.01 * np.random.default_rng(7).standard_normal(len(tp)))).astype(np.float32)
    _, _, rhs, _ = ctx.weight_data(G, tobs, tp)
    G.append_laplacian2d(nx, ny, np.array([c["weight_vs"]] * kmax + [c["weight_gcs"]] * (2 * kmax if azim else 0), np.float32))
    rhs = np.ascontiguousarray(rhs, np.float32)[:m_data]
    ng = (3 if azim else 1) * (nx - 2) * (ny - 2)
    calls = [] if posterior else [(K, True) for K in points] + [(max(points), False)]
    if posterior:
        runs = []
        for r in range(posterior + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.map_posterior(G, m_data, nx, ny, kmax, azim, c["damp"])
            runs.append(dict({k: ctx.stat(k) for k in POST_PARTS}, wall_s=time.perf_counter() - t0))
        out = {"case": name, "mode": "azim" if azim else "iso", "n_g": ng, "kmax": kmax, "calls": posterior, "n_failed": res["n_failed"]}
        out.update({k: float(np.median([x[k] for x in runs[1:]])) for k in runs[0]})
        print(json.dumps(out), flush=True)
    for K, full in calls:
        out = {"case": name, "mode": "azim" if azim else "iso", "n_g": ng, "kmax": kmax, "rays": int(m_data), "nnz": int(G.nnz), "K": K,
               "dof": full, "evidence": full, "workspace_GiB": (3 if full else 2) * ng * ng * 8 / 2 ** 30}
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.map_tradeoff(G, m_data, rhs, nx, ny, kmax, azim, factors(K), c["damp"], dof=full, evidence=full)
            out["wall_s"] = time.perf_counter() - t0
            out.update({k: ctx.stat(k) for k in PARTS})
            tot = res["total"]
            out.update(n_failed=int(res["n_failed"].sum()), pick_total=res["pick_total"], chi2=[float(v) for v in tot["chi2"]],
                       reg2=[float(v) for v in tot["reg2sum"]], mdata_p=[int(v) for v in res["mdata_p"]])
            if full:
                out.update(dof_sum=[float(v) for v in tot["dof"]], logev=[float(v) for v in tot["logev"]],
                           pick_gcv=[p["gcv"] for p in res["pick"]], pick_evidence=[p["evidence"] for p in res["pick"]],
                           pick_corner=[p["corner"] for p in res["pick"]])
        except Exception as e:                               # (a workspace that does not fit is a result, not a crash)
            out["error"] = str(e)
        print(json.dumps(out), flush=True)
    G.free()


def main():
    import dazimsurftomo_amd as dz
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="test4,s256")
    ap.add_argument("--modes", default="iso,azim")
    ap.add_argument("--points", default="1,9")
    ap.add_argument("--sources", type=int, default=1000)
    ap.add_argument("--receivers", type=int, default=32)
    ap.add_argument("--posterior", type=int, default=0)
    a = ap.parse_args()
    points = [int(v) for v in a.points.split(",")]
    ctx = dz.Context(0)
    for name in a.cases.split(","):
        if name == "test1":
            from tests.test_phase_map_program_gpu import inputs   # (test1's inputs from tests/golden/program_forward.npz, layer-mean MOD)
            c = example(inputs(maxiter=1, iso="F"), iso=False)
        elif name == "test4":
            c = example(golden_inputs("program_test4.npz"), iso=True)
        elif name == "s256":
            c = s256(a)
        else:
            raise SystemExit(f"unknown case {name}")
        for mode in a.modes.split(","):
            one_case(ctx, name, c, mode == "azim", points, a.posterior)
    ctx.close()


if __name__ == "__main__":
    main()
