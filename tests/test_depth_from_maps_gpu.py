"""-m gpu: the program SurfDepthFromMaps_amd (the second step of the two-step method) on the test1 synthetic data.

Its maps are the forward program's true maps in tests/golden/program_forward.npz: `out:period_Azm_tomo.real` has the format of
period_Azm_tomo_map.inv, and its columns 1-4 give period_phaseV_map.dat.  The starting MOD is the laterally uniform layer-mean model
of test_phase_map_program_gpu.py."""
import io
import os
import subprocess

import numpy as np

import pytest

from tests.test_phase_map_program_gpu import GOLD, KMAX, MAPS, NX, NY, build, inputs, run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = os.path.join(ROOT, "host", "SurfDepthFromMaps_amd")
NZ = 4
MAP_FILES = ("period_phaseV_map.dat", "period_Azm_tomo_map.inv", "period_map_coverage.dat", "para.in_map.log")


def true_maps():
    azm = str(np.load(GOLD)["out:period_Azm_tomo.real"])
    a = np.loadtxt(io.StringIO(azm), ndmin=2)
    c = "".join("%10.4f%10.4f%10.4f%10.4f\n" % tuple(row[:4]) for row in a)
    return {"period_phaseV_map.dat": c, "period_Azm_tomo_map.inv": azm}


def true_vs():
    vs = str(np.load(GOLD)["in:MODVs.true"]).split("\n")
    rows = np.array([[float(v) for v in line.split()] for line in vs[1:] if line.strip()])
    return rows.reshape(NZ, NY, NX)


def read_mod(path):
    lines = path.read_text().splitlines()
    depz = [float(v) for v in lines[0].split()]
    rows = np.array([[float(v) for v in line.split()] for line in lines[1:] if line.strip()])
    assert len(depz) == NZ and rows.shape == (NZ * NY, NX)
    return rows.reshape(NZ, NY, NX)


def log_rows(text):
    """the per-iteration lines of the log: iter, cells, rms_c_before, rms_c_after, max |dVs|"""
    out = []
    for line in text.splitlines():
        f = line.split()
        if len(f) == 5 and f[0].isdigit() and f[1].isdigit():
            out.append([float(v) for v in f])
    return np.array(out)


def nlines(path):
    return sum(1 for line in path.read_text().splitlines() if line.strip())


def inner_knot_rms(vs, truth):
    return float(np.sqrt(np.mean((vs[:-1, 1:-1, 1:-1] - truth[:-1, 1:-1, 1:-1]) ** 2)))


def check_outputs(d):
    """every output with its line count and format, Vs inside para.in's [2.0, 4.8]; returns (Vs, log rows, final RMS c misfit)"""
    log = (d / "para.in_2step.log").read_text()
    ncell = (NX - 2) * (NY - 2)
    assert nlines(d / "DSurfTomo_2step.inv") == NZ * NY * NX
    assert nlines(d / "MOD_2step") == 1 + NZ * NY
    assert nlines(d / "period_phaseV_2step.dat") == KMAX * ncell
    assert nlines(d / "Gc_Gs_model_2step.inv") == (NZ - 1) * ncell
    assert nlines(d / "period_Azm_tomo_2step.inv") == KMAX * ncell
    assert np.loadtxt(d / "Gc_Gs_model_2step.inv", ndmin=2).shape[1] == 8
    assert np.loadtxt(d / "period_Azm_tomo_2step.inv", ndmin=2).shape[1] == 9
    vs = read_mod(d / "MOD_2step")
    inv = np.loadtxt(d / "DSurfTomo_2step.inv", ndmin=2)
    assert np.allclose(inv[:, 3].reshape(NZ, NY, NX), vs, atol=1e-4)
    assert vs.min() >= 2.0 - 1e-4 and vs.max() <= 4.8 + 1e-4
    c = np.loadtxt(d / "period_phaseV_2step.dat", ndmin=2)
    c_true = np.loadtxt(io.StringIO(true_maps()["period_phaseV_map.dat"]), ndmin=2)
    assert np.allclose(c[:, :3], c_true[:, :3], atol=1e-3)
    final = [float(line.split()[-1]) for line in log.splitlines() if line.strip().startswith("final model:")]
    assert len(final) == 1, log
    return vs, log_rows(log), final[0]


def test_test1_true_maps_to_depth(tmp_path):
    """The issue's run: the layer-mean MOD, three iterations on the true maps of test1, iso-mode F, no coverage file.  Every output
    with its line count, Vs inside [2.0, 4.8], the log's c misfit falling every iteration and the final model's below half the
    start.  Measured on an MI355X: log c misfit 0.2001 -> 0.0620 -> 0.0404 km/s (final 0.0402); RMS(Vs - MODVs.true) over the inner cells and
    the inverted knots 0.1830 at the start -> 0.2857 km/s.  The Vs error grows because test1's true model varies laterally at its
    deepest knot (60 km: 3.82-4.58 km/s), which neither this program nor DAzimSurfTomo_amd inverts (dazim_model_update keeps the
    last knot): from the layer mean there, the three inverted knots absorb that structure to fit the 40 s map.  The Vs bar is
    therefore held on the run below, whose MOD carries the true deepest knot."""
    build()
    files = {**inputs(maxiter=3, iso="F"), **true_maps()}
    out = run(DEPTH, tmp_path, files)
    assert "Program finishes successfully" in out
    assert "period_map_coverage.dat is absent" in (tmp_path / "para.in_2step.log").read_text()
    vs, rows, final = check_outputs(tmp_path)
    assert rows.shape == (3, 5)
    assert (np.diff(rows[:, 2]) < 0).all() and (rows[:, 3] < rows[:, 2]).all() and final < 0.5 * rows[0, 2], rows
    truth = true_vs()
    e0, e1 = inner_knot_rms(read_mod_text(files["MOD"]), truth), inner_knot_rms(vs, truth)
    print("\n[measured] log c misfit before each iteration: " + " ".join("%.5f" % v for v in rows[:, 2]) + f", final {final:.5f}")
    print(f"[measured] RMS(Vs - MODVs.true), inner cells, inverted knots: start {e0:.4f} -> two-step {e1:.4f} km/s (not asserted)")


def test_test1_recovers_vs_with_the_true_deepest_knot(tmp_path):
    """The same run from a MOD whose inverted knots are the layer means and whose deepest knot is MODVs.true's: RMS(Vs - MODVs.true)
    over the inner cells and the inverted knots falls below the starting model's.  Measured on an MI355X: 0.1830 -> 0.0007 km/s;
    log c misfit 0.1562 -> 0.0074 -> 0.0005 km/s, final 0.00007 km/s."""
    build()
    files = {**inputs(maxiter=3, iso="F"), **true_maps()}
    start, truth = read_mod_text(files["MOD"]), true_vs()
    start[-1] = truth[-1]
    depz = files["MOD"].splitlines()[0]
    files["MOD"] = depz + "\n" + "".join(" ".join("%.4f" % v for v in row) + "\n" for row in start.reshape(NZ * NY, NX))
    run(DEPTH, tmp_path, files)
    vs, rows, final = check_outputs(tmp_path)
    assert (np.diff(rows[:, 2]) < 0).all() and final < rows[0, 2], rows
    e0, e1 = inner_knot_rms(start, truth), inner_knot_rms(vs, truth)
    print("\n[measured] log c misfit before each iteration: " + " ".join("%.5f" % v for v in rows[:, 2]) + f", final {final:.5f}")
    print(f"[measured] RMS(Vs - MODVs.true), inner cells, inverted knots: start {e0:.4f} -> two-step {e1:.4f} km/s")
    assert e1 < e0
    assert np.abs(vs[-1] - truth[-1]).max() <= 1e-4     # the deepest knot is kept


def read_mod_text(text):
    rows = np.array([[float(v) for v in line.split()] for line in text.splitlines()[1:] if line.strip()])
    return rows.reshape(NZ, NY, NX)


@pytest.mark.parametrize("iso", ["T", "F"])
def test_chained_after_surf_phase_maps(tmp_path, iso):
    """SurfPhaseMaps_amd, then SurfDepthFromMaps_amd in the same directory on its maps and coverage: the second completes and
    leaves the first program's files byte for byte as they were"""
    build()
    files = inputs(maxiter=2, iso=iso)
    run(MAPS, tmp_path, files)
    before = {n: (tmp_path / n).read_bytes() for n in MAP_FILES if (tmp_path / n).exists()}
    assert ("period_Azm_tomo_map.inv" in before) == (iso == "F") and "period_map_coverage.dat" in before
    out = run(DEPTH, tmp_path, files)
    assert "Program finishes successfully" in out
    assert "read period_map_coverage.dat" in (tmp_path / "para.in_2step.log").read_text()
    for n, b in before.items():
        assert (tmp_path / n).read_bytes() == b, n
    assert (tmp_path / "Gc_Gs_model_2step.inv").exists() == (iso == "F")
    assert nlines(tmp_path / "period_phaseV_2step.dat") == KMAX * (NX - 2) * (NY - 2)


def run_failing(d, files):
    d.mkdir(exist_ok=True)
    for name, text in files.items():
        (d / name).write_text(text)
    out = subprocess.run([DEPTH, "para.in"], cwd=d, timeout=300, capture_output=True, text=True)
    return out.returncode, out.stdout + out.stderr


def test_bad_inputs_stop_with_a_message(tmp_path):
    build()
    files = inputs(maxiter=1, iso="T")
    rc, text = run_failing(tmp_path / "missing", files)
    assert rc != 0 and "period_phaseV_map.dat is missing" in text, text
    maps = true_maps()
    bad = dict(files, **{"para.in": files["para.in"].replace("5 12 25 40", "5 12 25 41")}, **maps)
    rc, text = run_failing(tmp_path / "periods", bad)
    assert rc != 0 and "periods differ from para.in's" in text, text
    assert not (tmp_path / "periods" / "MOD_2step").exists()


def test_a_word_for_an_optional_argument_is_refused(tmp_path):
    """the checked parser of host/dazim_io.f90: a message naming the argument and a non-zero status, before anything is read"""
    build()
    files = dict(inputs(maxiter=1, iso="T"), **true_maps())
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    out = subprocess.run([DEPTH, "para.in", "2.0", "2.0", "small"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert out.returncode != 0 and " ERROR: argument 4 is not a number: small" in out.stdout.splitlines(), out.stdout + out.stderr
    assert not (tmp_path / "MOD_2step").exists()
