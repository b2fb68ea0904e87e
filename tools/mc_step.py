"""Times of the Monte-Carlo step (profiles/depth_mc.md).

    python tools/mc_step.py [--steps S] [--big N] [--proposal K] [--ntemp R [--tmax T]]
    python tools/mc_step.py --program [--dir D] [--proposal K] [--ntemp R [--tmax T]]
    python tools/mc_step.py --aniso N [--steps S] [--big N]
    python tools/mc_step.py --noise A0 B0 [--steps S] [--proposal K] [--ntemp R [--tmax T]]
    python tools/mc_step.py --program --noise A0 B0 [--dir D] [--proposal K] [--ntemp R [--tmax T]]
    python tools/mc_step.py --prior S D [--steps S] [--proposal K] [--ntemp R [--tmax T]] [--noise A0 B0]
    python tools/mc_step.py --program --prior S D [--dir D] [--proposal K] [--ntemp R [--tmax T]] [--noise A0 B0]
    python tools/mc_step.py --typed [--steps S] [--big N] [--runs R]
    python tools/mc_step.py --shapes [--noise A0 B0 | --groups] [--prior S D] [--steps S] [--big N] [--runs R]
    python tools/mc_step.py --radial [--steps S] [--runs R] [--proposal K]

On bench.py's S-256 model (54 x 54 columns: 2 704 inner cells, 12 knots, 16 periods) with 8, 32 and 64 chains per cell, and on an
N x N grid of the same model (default 202: 200 x 200 inner cells) with 8 chains: one dazim_mc_run of S steps (S/2 burn-in, S/2
recorded) after a 5-step warm-up run.  Reports ms per step -- the run's wall time ("mc"), its dispersion calls ("mc.disp"), its
k_mc_step launches ("mc.step") and the rest (host work of the calls) -- and curves per second.  One JSON line per case.

--program: the wall time of host/SurfDepthMC_amd's default run (2 000 burn-in + 2 000 recorded steps, 32 chains) at S-256.  The
inputs are written to D (default: a temporary directory): para.in with S-256's grid, knots, sublayers and periods, the model as MOD,
and its exact curves as period_phaseV_map.dat (no coverage file: every cell and period weighted).  One JSON line with the wall time
and the log's summary lines.

--proposal 1: the covariance-adapted proposal (dazim_mc_set_proposal) instead of the default 0.  The timed run then adapts every 5
burn-in steps instead of every 50, so that its S/2 burn-in steps hold factorisations and its recorded steps draw from the factor;
"cov_cells" counts the cells that did.

--ntemp R: parallel tempering with R rungs up to temperature T (dazim_mc_set_tempering; default T 16, a swap round every step)
instead of the default 1, no tempering; "swap_min" and "swap_med" are the run's swap acceptances over cells and rung pairs.

--aniso N: the Gc/Gs pass (dazim_mc_set_aniso, one pass per N recorded steps: gather, dispersion, TI kernels, column solves) at S-256
with 32 chains and on the big grid with 8: after a warm-up run that holds one pass, three runs of S recorded steps each; reports
the median over the runs of the ms of one pass ("mc.aniso" / "mc.aniso_passes") beside the ms of one step without its share of the
passes (profiles/depth_mc_aniso.md).

--noise A0 B0: the hierarchical noise scale (dazim_mc_set_noise, lambda^2 ~ InverseGamma(A0, B0)) at S-256 with 32 chains: five
pairs of runs of S steps, the mode off then on, alternating, each on a fresh handle after its own warm-up run; reports the ms per
step of the k_mc_step launches of every run and the medians of the five (profiles/depth_mc_noise.md).  With --program: the default
run with arguments 13 and 14, the log's noise lines among those kept.

--prior S D: the Gaussian smoothness prior (dazim_mc_set_prior, smooth S and damp D about the start model) at S-256 with 32 chains:
five pairs of runs, the prior off then on, alternating, as for --noise (with --noise the mode is on in both runs of a pair;
profiles/depth_mc_prior.md).  With --program: the default run with arguments 15 and 16, the log's prior lines among those kept.

--typed: typed data (dazim_mc_set_segments) at S-256 with 32 chains and on the big grid with 8: Rayleigh phase alone at the model's
16 periods (the default run above, through set_segments) and at every other one of them, then Rayleigh and Love, phase and group
velocities together at those 8 periods each (32 virtual periods; four times 16 would pass the sampler's 60); R runs (default 3) of S
steps per case, each on a fresh handle after its warm-up run; reports the ms per step of "mc", "mc.disp" and "mc.step" of every run.
At S-256 two more cases on the four types: the one noise scale (dazim_mc_set_noise) and one per type (dazim_mc_set_noise_groups),
whose "mc.step" are the two step kernels side by side (profiles/mc_typed.md).

--shapes: one mode of the step kernel at S-256 with 32 chains and on the big grid with 8, R runs (default 3) of S steps each on a
fresh handle after its warm-up run, for comparing two builds (DAZIM_LIB; profiles/mc_noise_once.md): the fixed noise level, --noise
A0 B0, or --groups, one noise scale per type on the four types of --typed (dazim_mc_set_noise_groups); each with --prior S D as well.
Reports the ms per step of "mc", "mc.disp" and "mc.step" of every run.

--radial: radial anisotropy (dazim_mc_set_radial, sigma_hv 0.2) at S-256 with 32 chains and the model's 16 periods as Rayleigh phase
and again as Love phase (32 virtual periods, 22 sampled knots): R runs (default 3) of S steps, each on a fresh handle after its warm-up
run, with the ms per step of "mc", "mc.disp" and "mc.step"; beside them, on the last handle's own two models, S repeats of the two
dazim_dispersion_kernels_typed calls alone: their wall time per repeat and the kernel timers' share (profiles/mc_radial.md)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_case(ctx, n, nchain, steps, proposal, ntemp, tmax, noise=None, prior=None):
    import bench
    bench.NX = bench.NY = n
    vel = bench.s256_model().astype(np.float32)
    depz, periods = np.asarray(bench.DEPZ, np.float32), np.asarray(bench.PERIODS, np.float64)
    nz, kmax, nlay = len(depz), len(periods), len(depz) - 1
    pv, _, _ = ctx.depthkernel(vel, depz, periods, bench.MINTHK, kernels=False)
    cobs = pv.reshape(kmax, n, n)[:, 1:-1, 1:-1].astype(np.float32)
    inner = vel[:nlay, 1:-1, 1:-1]
    vmin, vmax = (inner - 0.4).astype(np.float32), (inner + 0.4).astype(np.float32)
    wdat = np.full((kmax, n - 2, n - 2), 100.0, np.float32)
    mc = ctx.mc_create(n, n, nz, kmax, nchain, 100, 1, vel, vmin, vmax, cobs, wdat, nadapt=5 if proposal else 50, proposal=proposal,
                       ntemp=ntemp, tmax=tmax, noise=noise, prior=prior)
    mc.run(depz, bench.MINTHK, periods, 5, 0)                 # warm-up: code objects, scratch buffers
    nr = mc.run(depz, bench.MINTHK, periods, steps // 2, steps - steps // 2)
    wall, disp, stp = ctx.stat("mc"), ctx.stat("mc.disp"), ctx.stat("mc.step")
    r = mc.result()
    lam = mc.noise_result()["lam_mean"] if noise else None
    mc.free()
    ms = lambda s: 1e3 * s / steps
    return {"grid": f"{n}x{n} columns ({(n - 2) ** 2} inner cells), {nz} knots ({nlay} sampled), {kmax} periods", "nchain": nchain,
            "noise": list(noise) if noise else None, "median_lam_mean": float(np.median(lam)) if noise else None,
            "prior": list(prior) if prior else None,
            "proposal": proposal, "ntemp": ntemp, "swap_min": ctx.stat("mc.swap_min"), "swap_med": ctx.stat("mc.swap_med"),
            "cov_cells": int(ctx.stat("mc.cov_cells")), "steps": steps, "curves_per_step": mc.ncol, "ms_per_step": ms(wall),
            "disp_ms_per_step": ms(disp),
            "mc_step_ms_per_step": ms(stp), "other_ms_per_step": ms(wall - disp - stp), "mc_step_share": stp / wall,
            "curves_per_s": mc.ncol * steps / wall, "accept": ctx.stat("mc.accept"), "no_root": nr,
            "median_std_km_s": float(np.median(r["std"])), "median_rhat": float(np.nanmedian(r["rhat"]))}


def typed_case(ctx, n, nchain, steps, name, runs, prior=None):
    import bench
    bench.NX = bench.NY = n
    vel = bench.s256_model().astype(np.float32)
    depz, periods = np.asarray(bench.DEPZ, np.float32), np.asarray(bench.PERIODS, np.float64)
    nz, nlay = len(depz), len(depz) - 1
    kinds = {"rc16": [(2, 0, periods)], "rc8": [(2, 0, periods[::2])]}
    four = [(2, 0, periods[::2]), (2, 1, periods[::2]), (1, 0, periods[::2]), (1, 1, periods[::2])]
    segs = kinds.get(name, four)
    virt = np.concatenate([s[2] for s in segs])
    K = len(virt)
    pv, _, _ = ctx.dispersion_kernels_typed(vel, depz, segs, bench.MINTHK, kernels=False)
    cobs = pv.reshape(K, n, n)[:, 1:-1, 1:-1].astype(np.float32)
    inner = vel[:nlay, 1:-1, 1:-1]
    vmin, vmax = (inner - 0.4).astype(np.float32), (inner + 0.4).astype(np.float32)
    wdat = np.where(cobs != 0, np.float32(100.0), np.float32(0)).astype(np.float32)
    out = {"case": name, "grid": f"{n}x{n} columns ({(n - 2) ** 2} inner cells), {nz} knots ({nlay} sampled), {K} virtual periods",
           "segments": [(iw, ig, len(t)) for iw, ig, t in segs], "nchain": nchain, "steps": steps, "ms_per_step": [],
           "disp_ms_per_step": [], "mc_step_ms_per_step": []}
    for _ in range(runs):
        mc = ctx.mc_create(n, n, nz, K, nchain, 100, 1, vel, vmin, vmax, cobs, wdat)
        mc.set_segments(segs)
        if name == "four_noise":
            mc.set_noise(2.0, 1.0)
        elif name == "four_groups":
            mc.set_noise_groups(np.repeat(np.arange(4), K // 4), [2.0] * 4, [1.0] * 4)
        if prior:
            mc.set_prior(*prior)
        mc.run(depz, bench.MINTHK, virt, 5, 0)                    # warm-up: code objects, scratch buffers
        out["no_root"] = mc.run(depz, bench.MINTHK, virt, steps // 2, steps - steps // 2)
        for key, stat in (("ms_per_step", "mc"), ("disp_ms_per_step", "mc.disp"), ("mc_step_ms_per_step", "mc.step")):
            out[key].append(1e3 * ctx.stat(stat) / steps)
        out["curves_per_step"] = mc.ncol
        out["noise_groups"] = int(ctx.stat("mc.noise_groups"))
        mc.free()
    for key in ("ms_per_step", "disp_ms_per_step", "mc_step_ms_per_step"):
        out[key + "_median"] = float(np.median(out[key]))
    return out


def radial_case(ctx, steps, runs, proposal):
    import bench
    import torch
    n = bench.NX = bench.NY = 54
    vel = bench.s256_model().astype(np.float32)
    depz, periods = np.asarray(bench.DEPZ, np.float32), np.asarray(bench.PERIODS, np.float64)
    nz, nl = len(depz), len(depz) - 1
    segs = [(2, 0, periods), (1, 0, periods)]
    virt = np.concatenate([periods, periods])
    K = len(virt)
    pv, _, _ = ctx.dispersion_kernels_typed(vel, depz, segs, bench.MINTHK, kernels=False)
    cobs = pv.reshape(K, n, n)[:, 1:-1, 1:-1].astype(np.float32)
    wdat = np.where(cobs != 0, np.float32(100.0), np.float32(0)).astype(np.float32)
    vel0 = np.concatenate([vel[:nl], vel[:nl], vel[nl:]])
    inner = vel0[:-1, 1:-1, 1:-1]
    vmin, vmax = (inner - 0.4).astype(np.float32), (inner + 0.4).astype(np.float32)
    out = {"case": "radial", "grid": f"{n}x{n} columns ({(n - 2) ** 2} inner cells), {nl} + {nl} sampled knots, {K} virtual periods",
           "nchain": 32, "steps": steps, "proposal": proposal, "ms_per_step": [], "disp_ms_per_step": [], "mc_step_ms_per_step": []}
    sync = lambda: torch.cuda.synchronize(ctx.device)
    for r in range(runs):
        mc = ctx.mc_create(n, n, 2 * nl + 1, K, 32, 100, 1, vel0, vmin, vmax, cobs, wdat, nadapt=5 if proposal else 50, proposal=proposal,
                           segments=segs, radial=5.0)
        mc.run(depz, bench.MINTHK, virt, 5, 0)                    # warm-up: code objects, scratch buffers
        out["no_root"] = mc.run(depz, bench.MINTHK, virt, steps // 2, steps - steps // 2)
        for key, stat in (("ms_per_step", "mc"), ("disp_ms_per_step", "mc.disp"), ("mc_step_ms_per_step", "mc.step")):
            out[key].append(1e3 * ctx.stat(stat) / steps)
        out["curves_per_step"] = mc.ncol
        if r == runs - 1:                                         # the two typed calls alone, on the handle's own models
            vsv, vsh = (m.reshape(nl + 1, 1, -1) for m in mc.radial_models())
            walls, kern = [], 0.0
            for _ in range(steps):
                sync()
                t0 = time.perf_counter()
                ctx.dispersion_kernels_typed(vsv, depz, segs[:1], bench.MINTHK, kernels=False)
                kern += ctx.stat("disp")
                ctx.dispersion_kernels_typed(vsh, depz, segs[1:], bench.MINTHK, kernels=False)
                kern += ctx.stat("disp_typed")
                sync()
                walls.append(1e3 * (time.perf_counter() - t0))
            out["two_typed_calls_wall_ms_median"] = float(np.median(walls))
            out["two_typed_calls_kernel_ms"] = 1e3 * kern / steps
        mc.free()
    for key in ("ms_per_step", "disp_ms_per_step", "mc_step_ms_per_step"):
        out[key + "_median"] = float(np.median(out[key]))
    return out


def shape_cases(ctx, a):
    """--shapes: the mode given by --noise / --groups / --prior at the two shapes of profiles/mc_typed.md"""
    for n, nchain in ((54, 32), (a.big, 8)):
        if a.groups:
            out = typed_case(ctx, n, nchain, a.steps, "four_groups", a.runs, a.prior)
        else:
            runs = [one_case(ctx, n, nchain, a.steps, a.proposal, a.ntemp, a.tmax, tuple(a.noise) if a.noise else None,
                             tuple(a.prior) if a.prior else None) for _ in range(a.runs)]
            out = {k: runs[-1][k] for k in ("grid", "nchain", "noise", "proposal", "ntemp", "steps", "curves_per_step")}
            for key in ("ms_per_step", "disp_ms_per_step", "mc_step_ms_per_step"):
                out[key] = [r[key] for r in runs]
        out["prior"] = list(a.prior) if a.prior else None
        print(json.dumps(out), flush=True)


def noise_cases(ctx, steps, proposal, ntemp, tmax, noise, pairs=5, prior=None):
    """pairs of runs off / on of the noise mode or, with `prior`, of the prior (the noise mode then as given in both)"""
    runs = {"off": [], "on": []}
    for _ in range(pairs):
        for name in ("off", "on"):
            if prior:
                runs[name].append(one_case(ctx, 54, 32, steps, proposal, ntemp, tmax, tuple(noise) if noise else None,
                                           tuple(prior) if name == "on" else None))
            else:
                runs[name].append(one_case(ctx, 54, 32, steps, proposal, ntemp, tmax, tuple(noise) if name == "on" else None))
    out = dict(runs["on"][-1])
    for name in runs:
        for key in ("mc_step_ms_per_step", "ms_per_step", "disp_ms_per_step"):
            v = [r[key] for r in runs[name]]
            out[f"{key}_{name}"] = v
            out[f"{key}_{name}_median"] = float(np.median(v))
    out["median_std_km_s_off"] = runs["off"][-1]["median_std_km_s"]
    return out


def aniso_case(ctx, n, nchain, steps, nthin):
    import bench
    bench.NX = bench.NY = n
    vel = bench.s256_model().astype(np.float32)
    depz, periods = np.asarray(bench.DEPZ, np.float32), np.asarray(bench.PERIODS, np.float64)
    nz, kmax, nlay = len(depz), len(periods), len(depz) - 1
    pv, _, _ = ctx.depthkernel(vel, depz, periods, bench.MINTHK, kernels=False)
    lsen = ctx.ti_kernels(vel, depz, periods, bench.MINTHK, pv).reshape(nlay, kmax, n, n)[:, :, 1:-1, 1:-1].astype(np.float64)
    g = np.stack([0.02 * np.cos(0.4 * np.arange(nlay)), 0.015 * np.sin(0.3 * np.arange(nlay))])
    amap = np.einsum("lpji,rl->rpji", lsen, g).astype(np.float32)
    cobs = pv.reshape(kmax, n, n)[:, 1:-1, 1:-1].astype(np.float32)
    inner = vel[:nlay, 1:-1, 1:-1]
    vmin, vmax = (inner - 0.4).astype(np.float32), (inner + 0.4).astype(np.float32)
    wdat = np.full((kmax, n - 2, n - 2), 100.0, np.float32)
    mc = ctx.mc_create(n, n, nz, kmax, nchain, 100, 1, vel, vmin, vmax, cobs, wdat,
                       aniso=dict(nthin=nthin, amap=amap, wa=wdat, smooth=2.0, damp=0.0))
    mc.run(depz, bench.MINTHK, periods, 5, nthin)            # warm-up with one pass: code objects, scratch buffers
    pass_ms, step_ms = [], []
    for _ in range(3):
        mc.run(depz, bench.MINTHK, periods, 0, steps)
        wall, an, npass = ctx.stat("mc"), ctx.stat("mc.aniso"), ctx.stat("mc.aniso_passes")
        pass_ms.append(1e3 * an / max(npass, 1))
        step_ms.append(1e3 * (wall - an) / steps)
    r = mc.aniso_result()
    mc.free()
    return {"grid": f"{n}x{n} columns ({(n - 2) ** 2} inner cells), {nz} knots ({nlay} sampled), {kmax} periods", "nchain": nchain,
            "aniso_thin": nthin, "steps_per_run": steps, "passes_per_run": int(npass), "cold_columns": mc.ncol,
            "aniso_ms_per_pass": pass_ms, "aniso_ms_per_pass_median": float(np.median(pass_ms)),
            "ms_per_step_without_passes": step_ms, "ms_per_step_median": float(np.median(step_ms)),
            "skipped": int(ctx.stat("mc.aniso_skipped")), "median_std_between_over_std": float(np.nanmedian(r["std_between"] / r["std"]))}


PARA = """cccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccc
c INPUT PARAMETERS
cccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccc
surfphase_forward.dat                c: traveltime data file (not read)
{n} {n} {nz}                           c: nx ny nz
30.00 100.00                         c: goxd gozd
0.25 0.25                            c: dvxd dvzd
{sub}                                    c: number of sublayers
2.0 4.8                              c: minimum and maximum Vsv
10                                   c: max(sources, receivers)
0.4                                  c: sparsity fraction
1                                    c: maximum of iteration
T                                    c: iso-mode
cccccccc control parameters
2.0                                  c: smoothing for dVsv
2.0                                  c: smoothing for Gc,s
0.0                                  c: damping
cccccccccc periods
{kmax}                                   c: kmaxRc
{periods}
"""


def program_run(ctx, d, proposal, ntemp, tmax, noise=None, prior=None):
    import bench
    n = bench.NX = bench.NY = 54
    vel = bench.s256_model().astype(np.float32)
    depz, periods = np.asarray(bench.DEPZ, np.float32), np.asarray(bench.PERIODS, np.float64)
    nz, kmax = len(depz), len(periods)
    pv, _, nf = ctx.depthkernel(vel, depz, periods, bench.MINTHK, kernels=False)
    assert nf == 0
    pv = pv.reshape(kmax, n, n)
    ctx.close()                      # (the program opens the GPU itself)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "para.in"), "w") as f:
        f.write(PARA.format(n=n, nz=nz, sub=int(bench.MINTHK), kmax=kmax, periods=" ".join("%g" % t for t in periods)))
    with open(os.path.join(d, "MOD"), "w") as f:
        f.write(" ".join("%.1f" % z for z in depz) + "\n")
        for k in range(nz):
            for j in range(n):
                f.write(" ".join("%.4f" % vel[k, j, i] for i in range(n)) + "\n")
    with open(os.path.join(d, "period_phaseV_map.dat"), "w") as f:
        for t in range(kmax):
            for j in range(1, n - 1):
                for i in range(1, n - 1):
                    f.write("%10.4f%10.4f%10.4f%10.4f\n" % (100.0 + (j - 1) * 0.25, 30.0 - (i - 1) * 0.25, periods[t], pv[t, j, i]))
    exe = os.path.join(ROOT, "host", "SurfDepthMC_amd")
    t0 = time.perf_counter()
    args = ["2000", "32", "0", "0.01", "1", str(proposal)] if proposal or ntemp > 1 or noise or prior else []
    if ntemp > 1 or noise or prior:
        args += [str(ntemp), "%g" % tmax]
    if noise or prior:               # aniso_thin, smooth_gcs, sigma_a at their defaults, then noise_a0, noise_b0
        args += ["0", "2.0", "0.01"] + (["%g" % noise[0], "%g" % noise[1]] if noise else ["0", "1"])
    if prior:                        # smooth_vs, damp_vs
        args += ["%g" % prior[0], "%g" % prior[1]]
    out = subprocess.run([exe, "para.in"] + args, cwd=d, capture_output=True, text=True, timeout=1500)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    log = open(os.path.join(d, "para.in_mc.log")).read().splitlines()
    keep = [l.strip() for l in log if any(k in l for k in ("cells sampled", "without a root", "run", "acceptance", "R-hat", "rms_c", "proposal",
                                                                "covariance", "tempering", "ladder", "swap", "T = 1", "noise",
                                                                "Gaussian prior"))]
    return {"program": "SurfDepthMC_amd para.in (defaults: 2000 + 2000 steps, 32 chains)", "proposal": proposal, "ntemp": ntemp,
            "noise": list(noise) if noise else None, "prior": list(prior) if prior else None, "args": args,
            "grid": f"{n}x{n} columns ({(n - 2) ** 2} inner cells), {nz} knots, {kmax} periods",
            "wall_s": wall, "log": keep}


def main():
    import dazimsurftomo_amd as dz
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--big", type=int, default=202)
    ap.add_argument("--program", action="store_true")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--proposal", type=int, default=0, choices=(0, 1))
    ap.add_argument("--ntemp", type=int, default=1)
    ap.add_argument("--tmax", type=float, default=16.0)
    ap.add_argument("--aniso", type=int, default=0)
    ap.add_argument("--noise", type=float, nargs=2, default=None, metavar=("A0", "B0"))
    ap.add_argument("--prior", type=float, nargs=2, default=None, metavar=("S", "D"))
    ap.add_argument("--typed", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--groups", action="store_true")
    ap.add_argument("--radial", action="store_true")
    a = ap.parse_args()
    ctx = dz.Context(0)
    if a.radial:
        print(json.dumps(radial_case(ctx, a.steps, a.runs, a.proposal)), flush=True)
        ctx.close()
        return
    if a.shapes:
        shape_cases(ctx, a)
        ctx.close()
        return
    if a.typed:
        for n, nchain, names in ((54, 32, ("rc16", "rc8", "four", "four_noise", "four_groups")), (a.big, 8, ("rc16", "rc8", "four"))):
            for name in names:
                print(json.dumps(typed_case(ctx, n, nchain, a.steps, name, a.runs)), flush=True)
        ctx.close()
        return
    if a.aniso > 0:
        for n, nchain in ((54, 32), (a.big, 8)):
            print(json.dumps(aniso_case(ctx, n, nchain, a.steps, a.aniso)), flush=True)
        ctx.close()
        return
    if a.program:
        with tempfile.TemporaryDirectory() as tmp:
            print(json.dumps(program_run(ctx, a.dir or tmp, a.proposal, a.ntemp, a.tmax, a.noise, a.prior)), flush=True)
        return
    if a.prior:
        print(json.dumps(noise_cases(ctx, a.steps, a.proposal, a.ntemp, a.tmax, a.noise, prior=a.prior)), flush=True)
        ctx.close()
        return
    if a.noise:
        print(json.dumps(noise_cases(ctx, a.steps, a.proposal, a.ntemp, a.tmax, a.noise)), flush=True)
        ctx.close()
        return
    for n, nchain in ((54, 8), (54, 32), (54, 64), (a.big, 8)):
        print(json.dumps(one_case(ctx, n, nchain, a.steps, a.proposal, a.ntemp, a.tmax)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
