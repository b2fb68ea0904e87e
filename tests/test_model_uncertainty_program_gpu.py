"""-m gpu: DAzimSurfTomo_amd's second argument, uncertainty = 1 (model_uncertainty.dat from dazim_model_posterior on the last outer
iteration's matrix), on test1's inputs (tests/test_phase_map_program_gpu.py: 17 x 17 x 4, n = 675 in iso-mode T and 2 025 in F), two
iterations, in both iso-modes."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_depth_from_maps_gpu import DEPTH
from tests.test_phase_map_program_gpu import INV, MAPS, NX, NY, build, inputs, run

pytestmark = pytest.mark.gpu

NLAY = 3
NCELL = (NX - 2) * (NY - 2)
UNC = "model_uncertainty.dat"
LOG = "para.in_inv.log"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """per iso-mode: (directory of a run without the argument, directory of a run with uncertainty = 1, that run's stdout)"""
    build()
    out = {}
    for iso in ("T", "F"):
        plain, unc = tmp_path_factory.mktemp("plain" + iso), tmp_path_factory.mktemp("unc" + iso)
        run(INV, plain, inputs(maxiter=2, iso=iso))
        out[iso] = (plain, unc, run(INV, unc, inputs(maxiter=2, iso=iso), "1"))
    return out


@pytest.mark.parametrize("iso", ["T", "F"])
def test_uncertainty_file(runs, iso, tmp_path):
    """one line per inner cell and knot in Vs_resolution_2step.dat's order, 9 columns in iso-mode T and 14 in F, every value finite,
    std_noise <= std_post, leak in [0, 1]; the log's lines per knot.  Printed, not asserted: the median std_post of Vs per knot beside
    Vs_resolution_2step.dat's from the two-step programs on the same inputs (smoothing 2.0, sigma_c 0.02).  Measured on an MI355X, per
    knot from the top: iso-mode T direct 0.250, 0.125, 0.250 km/s; iso-mode F direct 0.250, 0.127, 0.250 against two-step 0.086, 0.063,
    0.047 km/s (the first and the last knot of the direct inversion are face cells of the Tikhonov rule: prior std 1 / (2 w) = 0.25)."""
    plain, unc, stdout = runs[iso]
    assert not (plain / UNC).exists()
    a = np.loadtxt(unc / UNC, ndmin=2)
    assert a.shape == (NLAY * NCELL, 9 if iso == "T" else 14) and len((unc / UNC).read_text().splitlines()) == NLAY * NCELL
    assert np.isfinite(a).all()
    assert (a[:, 3] > 0).all() and (a[:, 4] <= a[:, 3]).all() and (a[:, 4] >= 0).all() and (a[:, 7] >= 0).all() and (a[:, 8] >= 0).all()
    if iso == "F":
        assert (a[:, 9] > 0).all() and (a[:, 11] > 0).all() and (a[:, 13] >= 0).all() and (a[:, 13] <= 1).all()
    depths = np.unique(a[:, 2])
    assert len(depths) == NLAY and np.array_equal(a[:, 2], np.repeat(depths, NCELL))
    assert len(np.unique(a[:NCELL, :2], axis=0)) == NCELL and np.array_equal(a[:NCELL, :2], a[NCELL:2 * NCELL, :2])
    log = (unc / LOG).read_text()
    lines = [ln for ln in log.splitlines() if ln.startswith(" uncertainty depth")]
    assert len(lines) == NLAY and all("median std_post Vs" in ln for ln in lines) and "not factored" not in log
    assert all(("median leak Vs" in ln) == (iso == "F") for ln in lines)
    assert sum(ln.startswith(" uncertainty depth") for ln in stdout.splitlines()) == NLAY
    assert "uncertainty" not in (plain / LOG).read_text()
    direct = [float(np.median(a[k * NCELL:(k + 1) * NCELL, 3])) for k in range(NLAY)]
    print(f"\n[measured] iso-mode {iso}: median std_post of Vs per knot, direct inversion: " + " ".join(f"{v:.4e}" for v in direct) + " km/s")
    if iso == "F":                                           # the two-step programs on the same inputs
        run(MAPS, tmp_path, inputs(maxiter=2, iso=iso))
        run(DEPTH, tmp_path, {}, "2.0", "2.0", "0.02", "1")
        r = np.loadtxt(tmp_path / "Vs_resolution_2step.dat", ndmin=2)
        assert np.array_equal(r[:, :3], a[:, :3])            # the same cells and knots in the same order
        two = [float(np.median(r[k * NCELL:(k + 1) * NCELL, 4])) for k in range(NLAY)]
        print(f"\n[measured] iso-mode {iso}: median std_post of Vs per knot, two-step solve:     " + " ".join(f"{v:.4e}" for v in two) + " km/s")


@pytest.mark.parametrize("iso", ["T", "F"])
def test_other_files_are_byte_identical(runs, iso):
    plain, unc, _ = runs[iso]
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in unc.iterdir()) == sorted(names + [UNC])
    strip = lambda text: [ln for ln in text.splitlines() if "time cost" not in ln and not ln.startswith(" uncertainty")]
    for n in names:
        if n.endswith(".log"):
            assert strip((plain / n).read_text()) == strip((unc / n).read_text()), n
        else:
            assert (plain / n).read_bytes() == (unc / n).read_bytes(), n


def test_more_than_one_rank_is_refused(tmp_path):
    """the matrix of a multi-rank run is row-sharded: with the argument the program stops before any rank is started"""
    build()
    for name, text in inputs(maxiter=1, iso="T").items():
        (tmp_path / name).write_text(text)
    out = subprocess.run([INV, "para.in", "1"], cwd=tmp_path, timeout=300, capture_output=True, text=True, env=dict(os.environ, DAZIM_NGPU="2"))
    assert out.returncode != 0, out.stdout[-2000:]
    assert any(ln.startswith(" ERROR: uncertainty = 1 needs the whole matrix on one GPU") for ln in out.stdout.splitlines()), out.stdout[-2000:]
    assert not (tmp_path / "IterVel.out").exists() and not (tmp_path / UNC).exists()
