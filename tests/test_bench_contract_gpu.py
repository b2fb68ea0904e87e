"""-m gpu: bench.py keeps the driver's contract -- one JSON line, last on stdout, with the agreed keys -- on a reduced batch
(S-128 grid, 40 sources), single process and through torch.distributed.run with one rank (the N > 1 code path)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline"}
ARGS = ["--steps", "1", "--warmup", "1", "--workload", "s128", "--sources", "40", "--no-cpu"]


def check(stdout, steps=1):
    line = stdout.strip().splitlines()[-1]
    d = json.loads(line)
    assert KEYS <= set(d), KEYS - set(d)
    assert d["unit"] == "fields/s" and d["higher_is_better"] is True and d["vs_baseline"] is None and d["scaling"] == "weak"
    assert d["steps"] == steps and d["n_gpus"] == 1 and d["value"] > 0 and "workload" in d["config"]
    r = d["roofline"]
    # the eikonal kernel is bound by instruction issue: `achieved` / `frac` = the useful VALU instruction rate (the reference's
    # arithmetic x the pops the launch counted) against the measured issue peak -- ALWAYS numeric; `issue` = all VALU instructions
    # of the committed counter pass (null on this reduced batch, which has no pass); the HBM view sits under roofline.hbm
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic", "hbm", "issue"} <= set(r) and r["bound"] == "valu"
    assert r["achieved"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] < 1
    assert r["wave_pops_per_launch"] > 0 and 600 < r["peak"] < 700
    if r["issue"]["achieved"] is not None:
        assert r["frac"] < r["issue"]["frac"] < 1.2 and 0 < r["useful_frac_of_issued"] < 1
    h = r["hbm"]
    assert h["bound"] == "hbm" and abs(h["frac"] - h["achieved"] / h["peak"]) < 1e-12
    assert 0 < d["spmv"]["Ax"]["frac"] < 1 and 0 < d["spmv"]["ATy"]["frac"] < 1
    return d


def test_bench_single_process():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    check(out.stdout)


def test_bench_plain_run_leaves_the_full_legs_out():
    """without --full a run is set-up, warm-up, the timed steps and the line: no host-array step, no CPU baseline"""
    args = [t for t in ARGS if t != "--no-cpu"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = check(out.stdout)
    assert not {"value_host_api", "cpu_baseline", "forward_wall_s_per_step", "speedup_vs_cpu_1core_forward"} & set(d)


def test_bench_under_torchrun_one_rank():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                          "127.0.0.1", "--master-port", "29517", os.path.join(ROOT, "bench.py"), "--gpus", "1"] + ARGS,
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    check(out.stdout)


def test_bench_forced_row_sharded_solve():
    """DAZIM_BENCH_FORCE_DIST=1: process group + row-partitioned LSMR with all-reduces, the N > 1 path, on one rank"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", DAZIM_BENCH_FORCE_DIST="1", MASTER_PORT="29519")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = check(out.stdout)
    assert d["lsmr_iterations"] == 20


def test_bench_sweep_prints_one_line_per_count():
    """--sweep: the scaling curve in one command (here: the single count a 1-GPU box has)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sweep", "1"] + ARGS, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    check(lines[0])


def test_bench_dump_outputs_holds_the_last_timed_step(ctx, tmp_path):
    """--dump-outputs DIR: one float32 / float64 .npy per array the timed step returns, and --steps timed steps in the JSON line.  Every
    step of the bench starts from the same inputs (LSMR from x = 0), so the dumped arrays must be, bit for bit, the same step computed
    here through the library with bench.py's own inputs and options -- not read back from the bench's buffers."""
    import types
    import numpy as np
    import torch
    import bench
    import dazimsurftomo_amd as dz
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--workload", "s128",
                          "--sources", "40", "--no-cpu", "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = check(out.stdout, steps=2)
    names = ("x", "lsmr_info", "tpred", "pv", "sen_vs", "sen_vp", "sen_rho")
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{n}.npy" for n in names)
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in names}
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    # the step of bench.py's main(), one GPU, weak scaling
    bench.set_workload("s128")
    vel = bench.s256_model()
    scx, scz, per, fray, rcx, rcz, _ = bench.rank_workload(types.SimpleNamespace(sources=40, receivers=16, scaling="weak"), 0, 1)
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")
    d_vel, d_scx, d_scz, d_per = T(vel), T(scx), T(scz), T(per)
    c3, t_ir, t_ic, t_rw = bench.tikhonov_rows(bench.NX, bench.NY, len(bench.DEPZ), len(rcx), 2.0)
    b = np.concatenate([(np.random.default_rng(3).standard_normal(len(rcx)) * 0.5).astype(np.float32), np.zeros(c3, np.float32)])
    geo = (bench.NX, bench.NY, bench.GOXD, bench.GOZD, bench.DV, bench.DV)
    ctx.set_option("disp.async", 1)
    ctx.set_option("fmm.async", 1)
    try:
        pv, sen, nfail = ctx.depthkernel(d_vel, bench.DEPZ, bench.PERIODS, bench.MINTHK)
        g, nf = dz.geometry(*geo), len(scx)
        E = lambda shape, t=torch.float32: torch.empty(shape, dtype=t, device="cuda:0")
        fields = ctx.fmm_batch(*geo, pv, d_scx, d_scz, d_per, veln=E((len(bench.PERIODS), g.nnx, g.nnz)), ttnr=E((nf, 129, 129)),
                               nstsr=E((nf, 129, 129), torch.int32), boxes=E((nf, 12), torch.int32), status=E((nf,), torch.int32),
                               keep_fields=True)
        G, tpred, _ = ctx.rays_build_G(*geo, d_vel, fields, d_scx, d_scz, d_per, T(fray), T(rcx), T(rcz), sen)
        G.append_coo(c3, t_ir, t_ic, t_rw)
        x, info = ctx.lsmr(G, T(b), 0.01, 1e-9, 1e-9, 1e9, 20, 10)
        G.free()
    finally:
        ctx.set_option("disp.async", 0)
        ctx.set_option("fmm.async", 0)
    want = {"x": x, "tpred": tpred, "pv": pv, "sen_vs": sen[0], "sen_vp": sen[1], "sen_rho": sen[2]}
    for n, v in want.items():
        v = v.cpu().numpy()
        assert got[n].dtype == v.dtype and np.array_equal(got[n], v), n
    lsmr_info = [info[k] for k in ("istop", "itn", "normA", "condA", "normr", "normAr", "normx")]
    assert got["lsmr_info"].dtype == np.float64 and np.array_equal(got["lsmr_info"], np.array(lsmr_info, np.float64))
    assert got["lsmr_info"][1] == d["lsmr_iterations"] == 20 and nfail == 0 and np.abs(got["x"]).max() > 0
