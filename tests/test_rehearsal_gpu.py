"""-m gpu: the N-rank paths asserted on the ONE GPU a development / grading box has (file transport: every collective staged
through a directory, everything else the product path; RCCL itself needs one GPU per rank and is covered with one rank here and
with N >= 2 in tests/test_multigpu_gpu.py where GPUs exist).

* the model's dispersion / TI tables sharded over 2, 3 and 5 ranks inside the library (dazim_dispersion_kernels_sharded,
  dazim_ti_kernels_sharded: the reference's one parallel loop, OMP over the columns, inv/CalSurfG.f90:39-43, inv/depthkernelTI.f90)
  = the single-rank tables bit for bit, including ranks without a block and the deferred gather of the two-stream form;
* BASELINE config 5's shape rehearsed: `bench.py --gpus 5 --workload s512 --scaling strong` (reduced sources) with five ranks against
  the same bench with one rank -- predicted times and tables bit for bit, x to the LSMR bar;
* the RCCL transport and the file transport return the same bits (one rank: all a one-GPU box can run of RCCL)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world,ny", [(2, 7), (3, 7), (5, 4)])
def test_model_tables_sharded_over_ranks_are_bit_identical(tmp_path, world, ny):
    comm_dir = tmp_path / "comm"
    comm_dir.mkdir()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "shard_tables_worker.py"), str(r), str(world), str(comm_dir),
                               str(tmp_path / f"out{r}.npz"), str(ny)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[-2000:] for o in outs]
    for r in range(world):
        d = np.load(tmp_path / f"out{r}.npz")
        assert d["pv1"].min() > 0                                     # (a model with a root everywhere: the comparison means something)
        for name in ("pv_host", "pv_only", "pv_dev"):
            assert np.array_equal(d[name], d["pv1"]), (r, name)
        for q in range(3):
            assert np.abs(d[f"sen1_{q}"]).max() > 0
            assert np.array_equal(d[f"sen_host_{q}"], d[f"sen1_{q}"]), (r, q)
            assert np.array_equal(d[f"sen_dev_{q}"], d[f"sen1_{q}"]), (r, q)
        assert np.array_equal(d["sen_dev2_0"], d["sen1_0"]) and bool(d["sen_dev2_same"])
        assert int(d["nf_host"]) == int(d["nf1"]) == 0
        assert float(d["pending_after_call"]) == 1.0 and float(d["pending_after_sync"]) == 0.0   # the gather really was deferred
        assert np.array_equal(d["ls_host"], d["ls1"]) and np.array_equal(d["ls_dev"], d["ls1"]) and np.abs(d["ls1"]).max() > 0
        assert np.array_equal(d["gather"], np.array([[10.0 * q, 10.0 * q + 1] for q in range(world)], np.float32))
    assert sorted(os.listdir(comm_dir)) == []                          # the communicator leaves its directory as it found it


def run_bench(tmp_path, tag, world, args, port, opts=""):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if opts:
        env["DAZIM_OPTS"] = opts
    dump = str(tmp_path / tag)
    common = [os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "1", "--warmup", "0", "--no-cpu", "--dump", dump] + args
    if world == 1:
        out = subprocess.run([sys.executable] + common, capture_output=True, text=True, timeout=2400, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        stdout = out.stdout
    else:
        # the ranks are started here with the environment torch.distributed.run gives them (RANK, LOCAL_RANK, WORLD_SIZE, MASTER_*),
        # not under its agent, which opens the GPU as well: five ranks and this pytest process are six processes on the one GPU
        env.update(DAZIM_BENCH_REHEARSAL="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world))
        logs = [(open(tmp_path / f"{tag}.{r}.out", "w+"), open(tmp_path / f"{tag}.{r}.err", "w+")) for r in range(world)]
        procs = [subprocess.Popen([sys.executable] + common, stdout=o, stderr=e, text=True, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)))
                 for r, (o, e) in enumerate(logs)]
        try:
            for p in procs:
                p.wait(timeout=2400)
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
        text = []
        for o, e in logs:
            o.seek(0), e.seek(0)
            text.append((o.read(), e.read()))
            o.close(), e.close()
        assert all(p.returncode == 0 for p in procs), [(p.returncode, err[-3000:]) for p, (_, err) in zip(procs, text)]
        stdout = "".join(t for t, _ in text)
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                             # rank 0 alone prints
    return json.loads(lines[0]), [np.load(f"{dump}.{r}.npz") for r in range(world)]


# (fmm.ts=1: time slicing also for these small shards, so that the ray pass does run beside the eikonal launch on every rank -- by
# itself the library only does that for batches larger than the resident slots, the ones with a tail worth filling)
# (S-512 with five ranks, not config 5's eight: run as one job on a GPU node that stops a job holding the GPU in more than six
# processes, the eight-rank form -- eight ranks, the launcher's agent and pytest, ten processes -- was stopped there)
@pytest.mark.parametrize("workload,world,sources,opts", [("s512", 5, 40, "fmm.ts=1"), ("s512", 5, 40, "fmm.ts=1,fmm.ts_stages=2"), ("s128", 4, 60, "fmm.ts=1"),
                                                        ("s128", 4, 60, "fmm.ts=1,comm.gather_now=1"), ("s128", 4, 60, "")])
def test_bench_strong_scaling_n_ranks_against_one_rank(tmp_path, workload, world, sources, opts):
    """BASELINE config 5's shape (s512, strong scaling; five ranks, reduced source count) and a four-rank S-128, every rank on the one
    GPU: the N-rank run must reproduce the one-rank run of the same field list -- the dispersion tables (sharded by model rows,
    joined inside the library) and every ray's predicted time bit for bit (each is computed by exactly one rank with the same
    kernels), the LSMR solution to the bar of tests/bars.py for identical (A, b) (the ranks' partial products are added in rank
    order instead of one pass over all rows)."""
    args = ["--workload", workload, "--scaling", "strong", "--sources", str(sources), "--receivers", "12"]
    d1, r1 = run_bench(tmp_path, "one", 1, args, 0)
    # (opts "comm.gather_now=1": the sharded depth-kernel tables gathered at once instead of behind the perturbed copies -- what
    # the library does by itself over RCCL from four ranks on, so that the ray call may run beside the asynchronous eikonal launch)
    dn, rn = run_bench(tmp_path, "many", world, args, 29640 + world + len(opts) + (40 if workload == "s512" else 0), opts)
    if workload != "s512":    # (which heap form -- hence how many coarse stages, hence whether there is a tail worth filling -- a small S-512 shard gets is the library's choice)
        assert dn["rays_beside_eikonal_tail"] is ("fmm.ts=1" in opts)
    assert dn["n_gpus"] == world and dn["lsmr"]["rccl_nranks"] == world and dn["lsmr"]["collectives_per_iteration"] == 1
    assert dn["lsmr"]["collective"].startswith("all-gather") and dn["dispersion"].startswith("model rows sharded over the ranks inside the library")
    assert dn["lsmr_iterations"] == d1["lsmr_iterations"] == 20
    one = r1[0]
    nray = int(one["nray_all"])
    assert len(one["tpred"]) == nray
    tp = np.full(nray, np.nan, np.float32)
    for r in rn:
        assert np.array_equal(r["pv"], one["pv"]) and np.array_equal(r["sen_vs"], one["sen_vs"])
        assert np.array_equal(r["x"], rn[0]["x"])                     # replicated state: the same bits on every rank
        r0 = int(r["ray0"])
        assert np.all(np.isnan(tp[r0:r0 + len(r["tpred"])]))          # the shards do not overlap
        tp[r0:r0 + len(r["tpred"])] = r["tpred"]
    assert np.array_equal(tp, one["tpred"])                           # ... cover the list, and every time is the one-rank time
    x1, xn = one["x"], rn[0]["x"]
    assert np.linalg.norm(x1) > 0
    assert np.linalg.norm(xn - x1) <= 3e-4 * np.linalg.norm(x1), np.linalg.norm(xn - x1) / np.linalg.norm(x1)


def test_rccl_and_file_transport_return_the_same_bits(ctx, tmp_path):
    """One rank through RCCL (ncclAllGather on the library's stream) and one rank through files: both transports only move bytes and
    every sum over the ranks is formed by the same device kernel in rank order, so the two must agree bit for bit -- here with
    the one rank a one-GPU box can give RCCL; with N ranks the same holds by construction (csrc/comm.hip)."""
    import torch
    import dazimsurftomo_amd as dz
    from tests.dist_lsmr_worker import CFG, system
    m, n, irow, icol, rw, b = system()
    G = ctx.csr_from_coo(m, n, irow, icol, rw)
    d_b = torch.from_numpy(b).cuda()
    res = {}
    for kind in ("none", "rccl", "files", "rccl_allreduce"):
        if kind.startswith("rccl"):
            ctx.comm_init(1, 0, dz.comm_unique_id())
        elif kind == "files":
            d = tmp_path / "comm"
            d.mkdir()
            ctx.comm_init_files(1, 0, d)
        ctx.set_option("comm.allreduce", 1 if kind == "rccl_allreduce" else 0)
        x, info = ctx.lsmr(G, d_b, *CFG, x=torch.zeros(n, dtype=torch.float32, device="cuda:0"))
        h = ctx.comm_allreduce(np.array([1.5, -2.0], np.float32))
        g = ctx.comm_allgather(np.array([3, 4], np.int64))
        res[kind] = (x.cpu().numpy().copy(), info, h.copy(), g.copy(), ctx.stat("lsmr.collectives_per_iteration"), ctx.stat("lsmr.collective_kind"))
        if kind != "none":
            ctx.comm_free()
    ctx.set_option("comm.allreduce", 0)
    G.free()
    assert res["rccl"][4] == res["files"][4] == 1.0 and res["none"][4] == 0.0
    assert res["rccl"][5] == 1.0 and res["rccl_allreduce"][5] == 2.0
    for kind in ("files", "rccl_allreduce"):
        assert np.array_equal(res["rccl"][0], res[kind][0]) and res["rccl"][1] == res[kind][1], kind
    for kind in res:
        assert np.array_equal(res[kind][2], [1.5, -2.0]) and np.array_equal(res[kind][3].ravel(), [3, 4])
    # one rank of a sharded solve and the plain solve: the same products, the norm of u taken per shard first -> LSMR bars
    xs, xp = res["rccl"][0], res["none"][0]
    assert np.linalg.norm(xs - xp) <= 3e-4 * np.linalg.norm(xp) and abs(res["rccl"][1]["itn"] - res["none"][1]["itn"]) <= 3
