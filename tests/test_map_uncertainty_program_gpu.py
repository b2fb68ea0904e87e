"""-m gpu: SurfPhaseMaps_amd's fourth argument, uncertainty = 1 (period_map_uncertainty.dat from dazim_map_posterior on the last
iteration's matrix), and SurfDepthFromMaps_amd's sixth, map_sigma = 1 (Vs weights 1 / max(sigma_c, std_post) from that file), on
test1's inputs (tests/test_phase_map_program_gpu.py) in both iso-modes."""
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_depth_from_maps_gpu import DEPTH
from tests.test_phase_map_program_gpu import KMAX, MAPS, NX, NY, build, inputs, run

pytestmark = pytest.mark.gpu

NCELL = (NX - 2) * (NY - 2)
UNC = "period_map_uncertainty.dat"
DEPTH_FILES = ("DSurfTomo_2step.inv", "MOD_2step", "period_phaseV_2step.dat", "Gc_Gs_model_2step.inv", "period_Azm_tomo_2step.inv")


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """per iso-mode: (directory of a run without the argument, directory of a run with uncertainty = 1, that run's stdout)"""
    build()
    out = {}
    for iso in ("T", "F"):
        plain, unc = tmp_path_factory.mktemp("plain" + iso), tmp_path_factory.mktemp("unc" + iso)
        run(MAPS, plain, inputs(maxiter=2, iso=iso))
        out[iso] = (plain, unc, run(MAPS, unc, inputs(maxiter=2, iso=iso), "2.0", "2.0", "1"))
    return out


@pytest.mark.parametrize("iso", ["T", "F"])
def test_uncertainty_file(maps, iso):
    """one line per vertex and period in period_phaseV_map.dat's order, 8 columns in iso-mode T and 13 in F, every value finite,
    std_noise <= std_post, leak in [0, 1]; the log's lines per period.  Printed, not asserted: the median std_post of c over the
    cells with DWS below and above the period's median.  Measured on an MI355X (two iterations, smoothing 2.0, no damping): iso-mode T
    0.249 km/s below, 0.156 .. 0.169 above; iso-mode F 0.250 below, 0.253 .. 0.267 above: with ten stations the cells that rays
    cross are the ones where c trades off against a1, a2."""
    plain, unc, stdout = maps[iso]
    assert not (plain / UNC).exists()
    a = np.loadtxt(unc / UNC, ndmin=2)
    assert a.shape == (KMAX * NCELL, 8 if iso == "T" else 13) and len((unc / UNC).read_text().splitlines()) == KMAX * NCELL
    c = np.loadtxt(unc / "period_phaseV_map.dat", ndmin=2)
    assert np.array_equal(a[:, :3], c[:, :3])
    assert np.isfinite(a).all()
    assert (a[:, 3] > 0).all() and (a[:, 4] <= a[:, 3]).all() and (a[:, 4] >= 0).all() and (a[:, 7] >= 0).all()
    if iso == "F":
        assert (a[:, 8] > 0).all() and (a[:, 10] > 0).all() and (a[:, 12] >= 0).all() and (a[:, 12] <= 1).all()
    log = (unc / "para.in_map.log").read_text()
    lines = [ln for ln in log.splitlines() if ln.startswith(" uncertainty period")]
    assert len(lines) == KMAX and all("median std_post c" in ln for ln in lines) and "not factored" not in log
    assert all(("median leak c" in ln) == (iso == "F") for ln in lines)
    assert sum(ln.startswith(" uncertainty period") for ln in stdout.splitlines()) == KMAX
    assert "uncertainty" not in (plain / "para.in_map.log").read_text()
    cov = np.loadtxt(unc / "period_map_coverage.dat", ndmin=2)
    for t in range(KMAX):
        sl = slice(t * NCELL, (t + 1) * NCELL)
        lo = cov[sl, 3] <= np.median(cov[sl, 3])
        print(f"\n[measured] iso-mode {iso} period {a[sl, 2][0]:.0f} s: median std_post of c, DWS below / above the median: "
              f"{np.median(a[sl, 3][lo]):.4e} / {np.median(a[sl, 3][~lo]):.4e} km/s")


@pytest.mark.parametrize("iso", ["T", "F"])
def test_other_files_are_byte_identical(maps, iso):
    plain, unc, _ = maps[iso]
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in unc.iterdir()) == sorted(names + [UNC])
    strip = lambda text: [ln for ln in text.splitlines() if "time cost" not in ln and not ln.startswith(" uncertainty")]
    for n in names:
        if n.endswith(".log"):
            assert strip((plain / n).read_text()) == strip((unc / n).read_text()), n
        else:
            assert (plain / n).read_bytes() == (unc / n).read_bytes(), n


def test_depth_program_with_map_sigma(maps, tmp_path):
    """map_sigma = 1 completes on the maps run's files and its log names the weights' source; without the argument the files are
    those of a run in a directory that never held the uncertainty file; with the argument and without the file the run stops"""
    plain, unc, _ = maps["F"]
    before, default, sigma = tmp_path / "before", tmp_path / "default", tmp_path / "sigma"
    shutil.copytree(plain, before)
    shutil.copytree(unc, default)
    shutil.copytree(unc, sigma)
    run(DEPTH, before, {})
    run(DEPTH, default, {})
    for n in DEPTH_FILES:
        assert (before / n).read_bytes() == (default / n).read_bytes(), n
    assert "uncertainty" not in (default / "para.in_2step.log").read_text()
    out = run(DEPTH, sigma, {}, "2.0", "2.0", "0.01", "0", "1")
    log = (sigma / "para.in_2step.log").read_text()
    line = [ln for ln in log.splitlines() if ln.startswith(" period_map_uncertainty.dat: weight 1/max(sigma_c, std_post) on")]
    assert len(line) == 1 and line[0] in out.splitlines() and "Program finishes successfully" in out
    f = line[0].split()
    used = int(f[f.index("on") + 1])
    cov = np.loadtxt(sigma / "period_map_coverage.dat", ndmin=2)
    assert used == int((cov[:, 3] > 0).sum()) and int(f[f.index("pairs;") + 1]) <= used
    assert all((sigma / n).exists() for n in DEPTH_FILES)
    missing = subprocess.run([DEPTH, "para.in", "2.0", "2.0", "0.01", "0", "1"], cwd=before, timeout=300, capture_output=True, text=True)
    assert missing.returncode != 0 and " ERROR: period_map_uncertainty.dat is missing (SurfPhaseMaps_amd writes it)" in missing.stdout.splitlines()
