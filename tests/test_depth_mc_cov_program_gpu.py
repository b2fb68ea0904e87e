"""-m gpu: the program SurfDepthMC_amd with its proposal argument (covariance-adapted proposals) on the
fixtures and small arguments of test_depth_mc_program_gpu.py."""
import numpy as np
import pytest

from tests.test_depth_from_maps_gpu import NX, NY, NZ, nlines
from tests.test_depth_mc_program_gpu import MC, OUTS, true_knot_files
from tests.test_phase_map_program_gpu import KMAX, build, run

pytestmark = pytest.mark.gpu

EXTRA = ("proposal 1: shaped by the chains' covariance", "cells with an adapted covariance:")


def test_proposal_1_runs_and_logs(tmp_path):
    build()
    files, _, _ = true_knot_files()
    out = run(MC, tmp_path, files, "400", "16", "0", "0.01", "1", "1")
    assert "Program finishes successfully" in out
    log = (tmp_path / "para.in_mc.log").read_text()
    for key in EXTRA + ("cells sampled", "acceptance over cells", "R-hat", "Program finishes successfully"):
        assert key in log and key in out, key
    ncell = (NX - 2) * (NY - 2)
    line = [l for l in log.splitlines() if EXTRA[1] in l][0].split()
    nset, ns = int(line[-3]), int(line[-1])
    print(f"\n[measured] cells with an adapted covariance {nset} of {ns}")
    assert 0 < nset <= ns <= ncell
    assert nlines(tmp_path / "MOD_mc") == 1 + NZ * NY
    assert nlines(tmp_path / "DSurfTomo_mc.inv") == NZ * NY * NX
    assert np.genfromtxt(tmp_path / "Vs_posterior_mc.dat").shape == ((NZ - 1) * ncell, 10)
    assert np.loadtxt(tmp_path / "cell_mc.dat", ndmin=2).shape == (ncell, 5)
    assert nlines(tmp_path / "period_phaseV_mc.dat") == KMAX * ncell


def test_explicit_proposal_0_is_the_default(tmp_path):
    build()
    files, _, _ = true_knot_files()
    got = {}
    for name, args in (("default", ("30", "4", "0", "0.01", "7")), ("zero", ("30", "4", "0", "0.01", "7", "0"))):
        out = run(MC, tmp_path / name, files, *args)
        got[name] = {n: (tmp_path / name / n).read_bytes() for n in OUTS if n != "para.in_mc.log"}
        assert not any(key in out for key in EXTRA), name
    assert got["default"] == got["zero"]


def test_refused_proposal(tmp_path):
    from tests.test_depth_mc_program_gpu import run_failing
    build()
    files, _, _ = true_knot_files()
    rc, text = run_failing(tmp_path / "two", files, "10", "4", "0", "0.01", "1", "2")
    assert rc != 0 and "proposal must be 0 or 1" in text
    assert not (tmp_path / "two" / "MOD_mc").exists()
