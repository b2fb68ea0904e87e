"""-m gpu: the program SurfDepthMC_amd with its ntemp and tmax arguments (parallel tempering) on the fixtures
and small arguments of test_depth_mc_program_gpu.py."""
import numpy as np
import pytest

from tests.test_depth_from_maps_gpu import NX, NY, NZ, nlines
from tests.test_depth_mc_program_gpu import MC, OUTS, run_failing, true_knot_files
from tests.test_phase_map_program_gpu import KMAX, build, run

pytestmark = pytest.mark.gpu

EXTRA = ("parallel tempering:", "ladder, temperatures", "swap acceptance over (cell, rung pair)", "chains per cell at T = 1 (of")


def test_tempered_run_and_log(tmp_path):
    build()
    files, _, _ = true_knot_files()
    out = run(MC, tmp_path, files, "400", "16", "0", "0.01", "1", "1", "4", "8")
    assert "Program finishes successfully" in out
    log = (tmp_path / "para.in_mc.log").read_text()
    for key in EXTRA + ("cells sampled", "acceptance over cells", "R-hat", "Program finishes successfully"):
        assert key in log and key in out, key
    ladder = [float(v) for v in [l for l in log.splitlines() if EXTRA[1] in l][0].split(":")[1].split()]
    assert np.allclose(ladder, [1.0, 2.0, 4.0, 8.0], atol=1e-3)
    swap = [float(v) for v in [l for l in log.splitlines() if EXTRA[2] in l][0].split(":")[1].split()]
    cold = [l for l in log.splitlines() if EXTRA[3] in l][0].split()
    print(f"\n[measured] swap acceptance over (cell, rung pair): min {swap[0]:.3f}, quartiles {swap[1]:.3f} {swap[2]:.3f} {swap[3]:.3f}")
    assert len(swap) == 4 and 0 < swap[0] <= swap[1] <= swap[2] <= swap[3] <= 1
    assert "4" in cold and "16)" in cold
    ncell = (NX - 2) * (NY - 2)
    assert nlines(tmp_path / "MOD_mc") == 1 + NZ * NY
    assert nlines(tmp_path / "DSurfTomo_mc.inv") == NZ * NY * NX
    assert np.genfromtxt(tmp_path / "Vs_posterior_mc.dat").shape == ((NZ - 1) * ncell, 10)
    assert np.loadtxt(tmp_path / "cell_mc.dat", ndmin=2).shape == (ncell, 5)
    assert nlines(tmp_path / "period_phaseV_mc.dat") == KMAX * ncell


def test_explicit_ntemp_1_is_the_default(tmp_path):
    build()
    files, _, _ = true_knot_files()
    got = {}
    for name, args in (("default", ("30", "4", "0", "0.01", "7")), ("one", ("30", "4", "0", "0.01", "7", "0", "1", "16"))):
        out = run(MC, tmp_path / name, files, *args)
        got[name] = {n: (tmp_path / name / n).read_bytes() for n in OUTS if n != "para.in_mc.log"}
        assert not any(key in out for key in EXTRA), name
    assert got["default"] == got["one"]


def test_refused_ladders(tmp_path):
    build()
    files, _, _ = true_knot_files()
    rc, text = run_failing(tmp_path / "five", files, "10", "32", "0", "0.01", "1", "0", "5")
    assert rc != 0 and "ntemp must be 1..nchain and divide nchain" in text
    assert not (tmp_path / "five" / "MOD_mc").exists()
    rc, text = run_failing(tmp_path / "cold", files, "10", "32", "0", "0.01", "1", "0", "4", "0.5")
    assert rc != 0 and "tmax must be a finite temperature above 1" in text
    assert not (tmp_path / "cold" / "MOD_mc").exists()
