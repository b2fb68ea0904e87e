"""-m gpu: the program SurfDepthMC_amd (Monte-Carlo Vs per map cell) on the test1 fixtures of test_depth_from_maps_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_depth_from_maps_gpu import DEPTH, MAP_FILES, NX, NY, NZ, nlines, read_mod, read_mod_text, true_maps, true_vs
from tests.test_phase_map_program_gpu import KMAX, MAPS, build, inputs, run

pytestmark = pytest.mark.gpu

MC = os.path.join(os.path.dirname(DEPTH), "SurfDepthMC_amd")
OUTS = ("MOD_mc", "DSurfTomo_mc.inv", "Vs_posterior_mc.dat", "period_phaseV_mc.dat", "cell_mc.dat", "para.in_mc.log")


def true_knot_files():
    """test1's inputs with the true maps and a MOD whose deepest knot is MODVs.true's (the other knots the layer means)"""
    files = {**inputs(maxiter=3, iso="T"), **true_maps()}
    start, truth = read_mod_text(files["MOD"]), true_vs()
    start[-1] = truth[-1]
    depz = files["MOD"].splitlines()[0]
    files["MOD"] = depz + "\n" + "".join(" ".join("%.4f" % v for v in row) + "\n" for row in start.reshape(NZ * NY, NX))
    return files, start, truth


def test_true_maps_posterior_covers_the_truth(tmp_path):
    build()
    files, start, truth = true_knot_files()
    out = run(MC, tmp_path, files, "400", "16")
    assert "Program finishes successfully" in out
    ncell = (NX - 2) * (NY - 2)
    assert nlines(tmp_path / "MOD_mc") == 1 + NZ * NY
    assert nlines(tmp_path / "DSurfTomo_mc.inv") == NZ * NY * NX
    post = np.genfromtxt(tmp_path / "Vs_posterior_mc.dat")
    assert post.shape == ((NZ - 1) * ncell, 10)
    cells = np.loadtxt(tmp_path / "cell_mc.dat", ndmin=2)
    assert cells.shape == (ncell, 5)
    assert nlines(tmp_path / "period_phaseV_mc.dat") == KMAX * ncell
    assert np.loadtxt(tmp_path / "period_phaseV_mc.dat", ndmin=2).shape[1] == 4
    log = (tmp_path / "para.in_mc.log").read_text()
    for key in ("seed", "prior: uniform", "cells sampled", "proposals without a root", "acceptance over cells", "R-hat",
                "posterior-mean model: rms_c", "Program finishes successfully"):
        assert key in log, key
    vs = read_mod(tmp_path / "MOD_mc")
    inv = np.loadtxt(tmp_path / "DSurfTomo_mc.inv", ndmin=2)
    assert np.allclose(inv[:, 3].reshape(NZ, NY, NX), vs, atol=1e-4)
    assert vs.min() >= 2.0 - 1e-4 and vs.max() <= 4.8 + 1e-4
    assert np.abs(vs[-1] - truth[-1]).max() <= 1e-4
    mean = post[:, 3].reshape(NZ - 1, NY - 2, NX - 2)
    assert np.allclose(mean, vs[:-1, 1:-1, 1:-1], atol=1e-4)
    t = truth[:-1, 1:-1, 1:-1]
    lo, hi = post[:, 5].reshape(t.shape), post[:, 7].reshape(t.shape)
    inside = float(((lo <= t + 1e-4) & (t - 1e-4 <= hi)).mean())
    e0 = float(np.sqrt(np.mean((start[:-1, 1:-1, 1:-1] - t) ** 2)))
    e1 = float(np.sqrt(np.mean((mean - t) ** 2)))
    print(f"\n[measured] truth inside [p2.5, p97.5] for {inside:.3f} of the inner (cell, knot) pairs; RMS(Vs - MODVs.true) start "
          f"{e0:.4f} -> posterior mean {e1:.4f} km/s; median std {np.median(post[:, 4]):.4f} km/s; "
          f"acceptance {cells[:, 2].min():.3f}..{cells[:, 2].max():.3f}; max R-hat {np.nanmax(post[:, 9]):.3f}")
    assert inside >= 0.9
    assert e1 < e0


def test_seeds(tmp_path):
    build()
    files, _, _ = true_knot_files()
    got = []
    for name, seed in (("a", "7"), ("b", "7"), ("c", "8")):
        run(MC, tmp_path / name, files, "30", "4", "0", "0.01", seed)
        got.append({n: (tmp_path / name / n).read_bytes() for n in OUTS if n != "para.in_mc.log"})
    assert got[0] == got[1]
    assert got[0]["Vs_posterior_mc.dat"] != got[2]["Vs_posterior_mc.dat"]


def test_shared_directory(tmp_path):
    """after SurfPhaseMaps_amd and SurfDepthFromMaps_amd in one directory: their files stay byte for byte as they were"""
    build()
    files = inputs(maxiter=2, iso="T")
    run(MAPS, tmp_path, files)
    run(DEPTH, tmp_path, files)
    names = list(MAP_FILES) + ["MOD_2step", "DSurfTomo_2step.inv", "period_phaseV_2step.dat", "para.in_2step.log"]
    before = {n: (tmp_path / n).read_bytes() for n in names if (tmp_path / n).exists()}
    assert "MOD_2step" in before and "period_map_coverage.dat" in before
    out = run(MC, tmp_path, files, "20", "4")
    assert "Program finishes successfully" in out
    assert "read period_map_coverage.dat" in (tmp_path / "para.in_mc.log").read_text()
    for n, b in before.items():
        assert (tmp_path / n).read_bytes() == b, n


def run_failing(d, files, *args):
    d.mkdir(exist_ok=True)
    for name, text in files.items():
        (d / name).write_text(text)
    out = subprocess.run([MC, "para.in", *args], cwd=d, timeout=300, capture_output=True, text=True)
    return out.returncode, out.stdout + out.stderr


def test_bad_inputs_stop_with_a_message(tmp_path):
    build()
    files = inputs(maxiter=1, iso="T")
    maps = true_maps()
    cases = [
        ("missing", files, (), "period_phaseV_map.dat is missing"),
        ("periods", dict(files, **{"para.in": files["para.in"].replace("5 12 25 40", "5 12 25 41")}, **maps), (),
         "periods differ from para.in's"),
        ("nchain", dict(files, **maps), ("10", "65"), "nchain must be 1..64"),
        ("nsample", dict(files, **maps), ("0",), "nsample must be at least 1"),
        ("sigma", dict(files, **maps), ("10", "4", "0", "-1"), "sigma_c must be positive"),
        ("width", dict(files, **maps), ("10", "4", "-0.1"), "width must not be negative"),
        ("word", dict(files, **maps), ("ten",), "is not a number"),
    ]
    for name, f, args, msg in cases:
        rc, text = run_failing(tmp_path / name, f, *args)
        assert rc != 0 and msg in text, (name, text)
        assert not (tmp_path / name / "MOD_mc").exists(), name
