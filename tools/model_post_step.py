"""Where dazim_model_posterior's time goes, beside one LSMR solve of the same matrix (profiles/model_posterior.md).

    python tools/model_post_step.py [--cases test3,test4_iso,test4_joint,s256_iso] [--reps 5] [--sources S] [--receivers N]

Per case one outer iteration's matrix as the program builds it (dispersion tables, eikonal fields, ray rows, CalDdatSigma weights,
Tikhonov rows), one LSMR solve of it with the program's controls (host wall seconds), then dazim_model_posterior: the stats
model_post.gram, .factor, .inverse, .c, .rows and model_posterior, and the host wall seconds of the call.  A call under 10 s is repeated
and the medians of --reps calls are printed, a longer one is run once.  One JSON line per case.
  test3        the 17 x 17 x 4 example in iso-mode F (n = 2 025), data from tests/golden/program_forward.npz, the layer-mean MOD
  test4_iso    test4_Yunnan (38 x 42 x 18) in iso-mode T (n = 24 480), model and data from tests/golden/program_test4.npz
  test4_joint  the same in iso-mode F (n = 73 440): two n x n fp64 matrices are 86 GB
  s256_iso     the bench workload S-256 (54 x 54 x 12, n = 29 744), --sources x --receivers rays per period"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("model_post.gram", "model_post.factor", "model_post.inverse", "model_post.c", "model_post.rows", "model_posterior")
PI = np.float32(3.1415926535898)


def parse_para(text):
    """the values of a para.in (the text before 'c:' on every line that is no comment)"""
    v = [ln.split("c:")[0].split() for ln in text.splitlines() if not ln.startswith("c") and ln.strip()]
    nx, ny, nz = (int(x) for x in v[1])
    return dict(nx=nx, ny=ny, nz=nz, goxd=float(v[2][0]), gozd=float(v[2][1]), dvxd=float(v[3][0]), dvzd=float(v[3][1]),
                minthk=float(v[4][0]), weight_vs=float(v[10][0]), weight_gcs=float(v[11][0]), damp=float(v[12][0]),
                periods=np.array([float(x) for x in v[14]], np.float64))


def parse_mod(text, nx, ny, nz):
    lines = [ln for ln in text.splitlines() if ln.strip()]
    depz = np.array(lines[0].split(), np.float32)
    vel = np.array([[float(x) for x in ln.split()] for ln in lines[1:1 + nz * ny]], np.float32).reshape(nz, ny, nx)
    return depz, vel


def parse_data(text, kmax):
    """the traveltime data file (inv/Main_Jt.f90:268-318) as flat arrays in period -> source -> receiver order"""
    rad = lambda lat, lon: ((np.float32(90.0) - np.float32(lat)) * PI / np.float32(180.0), np.float32(lon) * PI / np.float32(180.0))
    per_period = [[] for _ in range(kmax)]
    for ln in text.splitlines():
        t = ln.split()
        if not t:
            continue
        if t[0] == "#":
            cur = (rad(float(t[1]), float(t[2])), [])
            per_period[int(t[3]) - 1].append(cur)
        else:
            cur[1].append(rad(float(t[0]), float(t[1])))
    fs, fz, fp, ray_f, rx, rz = [], [], [], [], [], []
    for k in range(kmax):
        for (sx, sz), recv in per_period[k]:
            f = len(fs)
            fs.append(sx); fz.append(sz); fp.append(k + 1)
            for x, z in recv:
                ray_f.append(f); rx.append(x); rz.append(z)
    a = lambda v, t: np.asarray(v, t)
    return a(fs, np.float32), a(fz, np.float32), a(fp, np.int32), a(ray_f, np.int32), a(rx, np.float32), a(rz, np.float32)


def example(texts, iso):
    """a case from the texts of a program's inputs: para.in, MOD and the traveltime data file para.in names"""
    p = parse_para(texts["para.in"])
    depz, vel = parse_mod(texts["MOD"], p["nx"], p["ny"], p["nz"])
    data = [k for k in texts if k.endswith(".dat")][0]
    return dict(p, depz=depz, vel=vel, survey=parse_data(texts[data], len(p["periods"])), joint=not iso)


def golden_inputs(npz):
    g = np.load(os.path.join(ROOT, "tests", "golden", npz))
    return {k[3:]: str(g[k]) for k in g.files if k.startswith("in:")}


def s256(a):
    import bench
    bench.set_workload("s256")
    scx, scz, per, fray, rcx, rcz = bench.workload(a.sources, a.receivers, 0)
    return dict(nx=bench.NX, ny=bench.NY, nz=len(bench.DEPZ), goxd=bench.GOXD, gozd=bench.GOZD, dvxd=bench.DV,
                dvzd=bench.DV, minthk=bench.MINTHK, weight_vs=20.0, weight_gcs=30.0, damp=0.0, periods=np.asarray(bench.PERIODS, np.float64),
                depz=np.asarray(bench.DEPZ, np.float32), vel=bench.s256_model(), survey=(scx, scz, per, fray, rcx, rcz), joint=False)


def one_case(ctx, name, c, reps):
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
    b = np.concatenate([rhs, np.zeros(G.m - m_data, np.float32)])
    ctrl = (1e-5, 1e-4, 200.0, 500, 10) if joint else (1e-3, 1e-3, 1200.0, 1000, G.n // 4)   # host/dazim_main.f90
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, info = ctx.lsmr(G, b, c["damp"], *ctrl)
    lsmr_s = time.perf_counter() - t0
    out = {"case": name, "n": int(G.n), "rays": int(m_data), "nnz": int(G.nnz), "damp": c["damp"], "lsmr_wall_s": lsmr_s, "lsmr_itn": info["itn"],
           "workspace_GiB": 2 * G.n * G.n * 8 / 2 ** 30}
    runs = []
    try:
        for r in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.model_posterior(G, m_data, nx, ny, nz, joint, c["damp"], depz=c["depz"][:nz - 1])
            wall = time.perf_counter() - t0
            runs.append(dict({k: ctx.stat(k) for k in PARTS}, wall_s=wall))
            if wall >= 10.0:
                break
        out.update({k: float(np.median([x[k] for x in runs])) for k in runs[0]})
        out.update(calls=len(runs), n_failed=res["n_failed"],
                   median_std_post_vs_per_knot=[float(np.median(res["std_post"][0, k])) for k in range(nz - 1)],
                   median_width_h=float(np.median(res["width_h"][0])), median_width_z=float(np.median(res["width_z"][0])))
    except Exception as e:                                   # (a workspace that does not fit is a result, not a crash)
        out["error"] = str(e)
    print(json.dumps(out), flush=True)
    G.free()


def main():
    import dazimsurftomo_amd as dz
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="test3,test4_iso,test4_joint,s256_iso")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sources", type=int, default=1000)
    ap.add_argument("--receivers", type=int, default=32)
    a = ap.parse_args()
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
        one_case(ctx, name, c, a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
