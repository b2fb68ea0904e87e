"""-m gpu: the map-inversion program SurfPhaseMaps_amd end to end on the test1 synthetic data (tests/golden/program_forward.npz:
the forward program's surfphase_forward.dat from MODVs/MODGc/MODGs.true, and its true period maps period_Azm_tomo.real), started
from a laterally uniform MOD made of the layer means of MODVs.true."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = os.path.join(ROOT, "host", "SurfPhaseMaps_amd")
INV = os.path.join(ROOT, "host", "DAzimSurfTomo_amd")
GOLD = os.path.join(ROOT, "tests", "golden", "program_forward.npz")
NX = NY = 17
KMAX = 4

PARA = """cccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccc
c INPUT PARAMETERS
cccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccc
surfphase_forward.dat                c: traveltime data file
17 17 4                              c: nx ny nz
26.50  101.25                        c: goxd gozd
0.25 0.25                            c: dvxd dvzd
2                                    c: number of sublayers
2.0 4.8                              c: minimum and maximum Vsv
10                                   c: max(sources, receivers)
0.4                                  c: sparsity fraction
{maxiter}                                    c: maximum of iteration
{iso}                                    c: iso-mode
cccccccc control parameters
2.0                                  c: smoothing for dVsv
2.0                                  c: smoothing for Gc,s
0.0                                  c: damping
cccccccccc periods
4                                    c: kmaxRc
5 12 25 40
"""


def inputs(maxiter=3, iso="F"):
    g = np.load(GOLD)
    vs = str(g["in:MODVs.true"]).split("\n")
    depz = vs[0]
    rows = np.array([[float(v) for v in line.split()] for line in vs[1:] if line.strip()])
    nz = len(depz.split())
    assert rows.shape == (nz * NY, NX)
    mean = rows.reshape(nz, NY, NX).mean(axis=(1, 2))
    mod = depz + "\n" + "".join((" ".join("%.4f" % mean[k] for _ in range(NX)) + "\n") * NY for k in range(nz))
    return {"para.in": PARA.format(maxiter=maxiter, iso=iso), "MOD": mod, "surfphase_forward.dat": str(g["out:surfphase_forward.dat"])}


def build():
    import dazimsurftomo_amd as dz
    dz.build()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "all"])


def run(exe, d, files, *args):
    d.mkdir(exist_ok=True)
    for name, text in files.items():
        if not (d / name).exists():
            (d / name).write_text(text)
    out = subprocess.run([exe, "para.in", *args], cwd=d, timeout=900, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def table(path, ncol):
    a = np.loadtxt(path, ndmin=2)
    assert a.shape == (KMAX * (NX - 2) * (NY - 2), ncol), a.shape
    return a


def test_test1_end_to_end(tmp_path):
    """all four outputs with their column counts, one row per vertex and period; bias in [0, 1]; the recovered c closer to the
    true maps than the starting maps at every period (RMS over the cells with DWS above the period's median).
    Measured on an MI355X: c RMS error start -> recovered 0.201 -> 0.046, 0.218 -> 0.076, 0.258 -> 0.064, 0.263 -> 0.085 km/s at
    5, 12, 25, 40 s.  The a1/a2 correlation with the true maps is printed but not asserted: measured 0.07, 0.29, -0.07, -0.30.
    test1's true 2-psi terms are 0.004-0.017 km/s on average, five to ten times below the c error left after three iterations
    with ten stations, so this geometry does not resolve them.  The 2-psi recovery is asserted on a denser synthetic in
    test_phase_maps_gpu.py (correlation 0.93)."""
    build()
    run(MAPS, tmp_path / "start", inputs(maxiter=0))
    start = table(tmp_path / "start" / "period_phaseV_map.dat", 4)
    out = run(MAPS, tmp_path / "run", inputs())
    d = tmp_path / "run"
    c = table(d / "period_phaseV_map.dat", 4)
    azm = table(d / "period_Azm_tomo_map.inv", 9)
    cov = table(d / "period_map_coverage.dat", 5)
    log = (d / "para.in_map.log").read_text()
    assert sum(1 for line in log.splitlines() if line.split()[:1] in (["1"], ["2"], ["3"])) == 3, log
    assert "Program finishes successfully" in out
    assert ((cov[:, 4] >= 0) & (cov[:, 4] <= 1)).all() and (cov[:, 3] >= 0).all() and cov[:, 3].max() > 0
    truth = np.loadtxt(__import__("io").StringIO(str(np.load(GOLD)["out:period_Azm_tomo.real"])), ndmin=2)
    assert truth.shape == azm.shape
    for a in (c, azm, cov, start):
        assert np.allclose(a[:, :3], truth[:, :3], atol=1e-3)          # lon, lat, period: the same vertices in the same order
    for t in range(KMAX):
        sl = slice(t * (NX - 2) * (NY - 2), (t + 1) * (NX - 2) * (NY - 2))
        good = cov[sl, 3] > np.median(cov[sl, 3])
        rms_start = np.sqrt(np.mean((start[sl, 3][good] - truth[sl, 3][good]) ** 2))
        rms_rec = np.sqrt(np.mean((c[sl, 3][good] - truth[sl, 3][good]) ** 2))
        print(f"\n[measured] period {truth[sl, 2][0]:.0f} s: c RMS error start {rms_start:.4f} -> recovered {rms_rec:.4f} km/s")
        assert rms_rec < rms_start
        av = np.concatenate([azm[sl, 7][good], azm[sl, 8][good]])
        at = np.concatenate([truth[sl, 7][good], truth[sl, 8][good]])
        r = float((av * at).sum() / np.sqrt((av * av).sum() * (at * at).sum()))
        print(f"[measured] period {truth[sl, 2][0]:.0f} s: a1/a2 correlation {r:.3f} (not asserted, see the docstring)")


def test_iso_mode_writes_no_anisotropy_map(tmp_path):
    build()
    run(MAPS, tmp_path, inputs(maxiter=2, iso="T"))
    assert not (tmp_path / "period_Azm_tomo_map.inv").exists()
    table(tmp_path / "period_phaseV_map.dat", 4)
    cov = table(tmp_path / "period_map_coverage.dat", 4)
    assert (cov[:, 3] >= 0).all() and cov[:, 3].max() > 0


def test_both_programs_in_one_directory_leave_the_3d_files_alone(tmp_path):
    """the 3-D program's files after a map run in the same directory equal those of a run on its own (lines with a wall time
    aside)"""
    build()
    files = inputs(maxiter=2)
    run(INV, tmp_path / "alone", files)
    run(INV, tmp_path / "both", files)
    run(MAPS, tmp_path / "both", files)
    names = sorted(n for n in os.listdir(tmp_path / "alone") if n not in files)
    assert "period_Azm_tomo.inv" in names and "period_phaseVMOD.dat" in names
    strip = lambda text: [line for line in text.splitlines() if "time cost" not in line]
    for n in names:
        a = (tmp_path / "alone" / n).read_text(errors="replace")
        b = (tmp_path / "both" / n).read_text(errors="replace")
        assert strip(a) == strip(b), n


def test_a_word_for_an_optional_argument_is_refused(tmp_path):
    """the checked parser of host/dazim_io.f90: a message naming the argument and a non-zero status, before the data file is read"""
    build()
    for name, text in inputs(maxiter=1).items():
        (tmp_path / name).write_text(text)
    out = subprocess.run([MAPS, "para.in", "smooth"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert out.returncode != 0 and " ERROR: argument 2 is not a number: smooth" in out.stdout.splitlines(), out.stdout + out.stderr
    assert not (tmp_path / "period_phaseV_map.dat").exists()
