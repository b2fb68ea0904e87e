"""Where dazim_model_tradeoff's time goes (profiles/model_tradeoff.md).

    python tools/model_tradeoff_step.py [--cases test3,test4_iso,s256_iso] [--points 1,9] [--sources S] [--receivers N]

Per case one outer iteration's matrix and weighted right-hand side as the program builds them (tools/model_post_step.py's cases), then
dazim_model_tradeoff with the program's factors 10^(-1 + 2k/(K-1)) on every block and para.in's damping, for each K of --points (K = 1:
the factor 1 alone), with dof and the evidence, and for the largest K once more without either.  Per call the stats model_trade.gram
(once per call: it must not grow with K), .factor, .solve, .inverse and model_tradeoff, the host wall seconds, and the three picks.
One JSON line per call."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.model_post_step import example, golden_inputs, s256   # noqa: E402

PARTS = ("model_trade.gram", "model_trade.factor", "model_trade.solve", "model_trade.inverse", "model_tradeoff")


def factors(K):
    return np.ones(1, np.float32) if K == 1 else (10.0 ** (-1.0 + 2.0 * np.arange(K) / (K - 1))).astype(np.float32)


def one_case(ctx, name, c, points):
    import torch
    nx, ny, nz, joint = c["nx"], c["ny"], c["nz"], c["joint"]
    geo = (nx, ny, c["goxd"], c["gozd"], c["dvxd"], c["dvzd"])
    scx, scz, per, ray_f, rx, rz = c["survey"]
    pv, sen, nfail = ctx.depthkernel(c["vel"], c["depz"], c["periods"], c["minthk"])
    lsen = ctx.ti_kernels(c["vel"], c["depz"], c["periods"], c["minthk"], pv) if joint else None
    fields = ctx.fmm_batch(*geo, pv, scx, scz, per)
    G, tp, _ = ctx.rays_build_G(*geo, c["vel"], fields, scx, scz, per, ray_f, rx, rz, sen, lsen=lsen)
    del fields
    m_data = G.m
    tp = np.asarray(tp).copy()
    tobs = (tp * (1.0 + 0.01 * np.random.default_rng(7).standard_normal(len(tp)))).astype(np.float32)
    _, _, rhs, _ = ctx.weight_data(G, tobs, tp)
    G.append_tikhonov(nx, ny, nz, np.array([c["weight_vs"]] + [c["weight_gcs"]] * (2 if joint else 0), np.float32))
    rhs = np.ascontiguousarray(rhs, np.float32)[:m_data]
    calls = [(K, True) for K in points] + [(max(points), False)]
    for K, full in calls:
        out = {"case": name, "n": int(G.n), "rays": int(m_data), "nnz": int(G.nnz), "K": K, "dof": full, "evidence": full,
               "workspace_GiB": (3 if full else 2) * G.n * G.n * 8 / 2 ** 30}
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.model_tradeoff(G, m_data, rhs, nx, ny, nz, joint, factors(K), c["damp"], dof=full, evidence=full)
            out["wall_s"] = time.perf_counter() - t0
            out.update({k: ctx.stat(k) for k in PARTS})
            out.update(n_failed=int(res["n_failed"].sum()), pick=res["pick"], chi2=[float(v) for v in res["chi2"]],
                       reg2=[float(v) for v in res["reg2"].sum(axis=1)])
            if full:
                out.update(dof_sum=[float(v) for v in res["dof"].sum(axis=1)], logev=[float(v) for v in res["logev"]])
        except Exception as e:                               # (a workspace that does not fit is a result, not a crash)
            out["error"] = str(e)
        print(json.dumps(out), flush=True)
    G.free()


def main():
    import dazimsurftomo_amd as dz
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="test3,test4_iso,s256_iso")
    ap.add_argument("--points", default="1,9")
    ap.add_argument("--sources", type=int, default=1000)
    ap.add_argument("--receivers", type=int, default=32)
    a = ap.parse_args()
    points = [int(v) for v in a.points.split(",")]
    ctx = dz.Context(0)
    for name in a.cases.split(","):
        if name == "test3":
            from tests.test_phase_map_program_gpu import inputs   # (test1's inputs from tests/golden/program_forward.npz, layer-mean MOD)
            c = example(inputs(maxiter=1, iso="F"), iso=False)
        elif name in ("test4_iso", "test4_joint"):
            c = example(golden_inputs("program_test4.npz"), iso=name == "test4_iso")
        elif name == "s256_iso":
            c = s256(a)
        else:
            raise SystemExit(f"unknown case {name}")
        one_case(ctx, name, c, points)
    ctx.close()


if __name__ == "__main__":
    main()
