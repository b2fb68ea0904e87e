"""-m gpu: SurfDepthFromMaps_amd's fifth argument, resolution = 1: Vs_resolution_2step.dat and Gc_Gs_resolution_2step.dat
(dazim_column_resolution on the final model) on the small test1 fixture of tests/test_depth_from_maps_gpu.py in iso-mode F.

The files against the Python call on MOD_2step's model with the program's weights and regularisers, the other outputs byte for byte
those of a run without the argument, no new file without it, and a refused value.

MOD_2step holds Vs to 4 decimals, and that alone moves the numbers past their printed precision (measured on an MI355X after two
iterations: std_post by 1.2e-5 of 0.097 km/s, rdiag by 7.8e-5, width by 5.8e-3 km).  So the values are compared on a third run that
starts from that MOD_2step with no iteration: there the program and Python hold the same fp32 model, and the files must equal the
Python call to half a unit of the last printed digit."""
import subprocess

import numpy as np
import pytest

from tests.test_depth_from_maps_gpu import DEPTH, NZ, nlines, read_mod, true_maps
from tests.test_phase_map_program_gpu import KMAX, NX, NY, build, inputs, run

pytestmark = pytest.mark.gpu

NLAY, NCELL = NZ - 1, (NX - 2) * (NY - 2)
NEW = ("Vs_resolution_2step.dat", "Gc_Gs_resolution_2step.dat")
OTHERS = ("DSurfTomo_2step.inv", "MOD_2step", "period_phaseV_2step.dat", "Gc_Gs_model_2step.inv", "period_Azm_tomo_2step.inv")
TRC = np.array([5.0, 12.0, 25.0, 40.0])
SMOOTH_VS, SMOOTH_GCS, SIGMA_C = 2.0, 1.5, 0.02                # (the damping is para.in's)
# one unit of the last printed digit per column (std_post std_noise rdiag rsum width)
QUANTUM = np.array([1e-5, 1e-5, 1e-4, 1e-4, 1e-2])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    build()
    files = {**inputs(maxiter=2, iso="F"), **true_maps()}
    plain, res = tmp_path_factory.mktemp("plain"), tmp_path_factory.mktemp("resolution")
    run(DEPTH, plain, files, str(SMOOTH_VS), str(SMOOTH_GCS), str(SIGMA_C))
    run(DEPTH, res, files, str(SMOOTH_VS), str(SMOOTH_GCS), str(SIGMA_C), "1")
    exact = tmp_path_factory.mktemp("exact")
    files0 = dict(files, **{"para.in": inputs(maxiter=0, iso="F")["para.in"], "MOD": (res / "MOD_2step").read_text()})
    out = run(DEPTH, exact, files0, str(SMOOTH_VS), str(SMOOTH_GCS), str(SIGMA_C), "1")
    return plain, res, exact, files0, out


def para_damping(text):
    line = [ln for ln in text.splitlines() if "damp" in ln.lower()]
    assert len(line) == 1, line
    return float(line[0].split()[0])


def test_without_the_argument_nothing_new(runs):
    plain, res, _, _, _ = runs
    for n in NEW:
        assert not (plain / n).exists() and (res / n).exists(), n
    assert "resolution" not in (plain / "para.in_2step.log").read_text()


def test_other_outputs_are_byte_identical(runs):
    plain, res, _, _, _ = runs
    for n in OTHERS:
        assert (plain / n).read_bytes() == (res / n).read_bytes(), n


def test_files_equal_the_python_call(runs, ctx):
    """(nz - 1) * ncell lines of 9 / 8 columns in DSurfTomo_2step.inv's cell order, after two iterations and on the run without
    one; on the latter the five numbers against Context.column_resolution with kernels at MOD_2step's model, w = 1 / sigma_c where
    the final model has a curve (no coverage file), the program's smoothing and para.in's damping, to half a unit of the last
    printed digit; the two log lines"""
    _, iterated, res, files, out = runs
    for name, ncol in zip(NEW, (9, 8)):
        a = np.loadtxt(iterated / name, ndmin=2)
        inv = np.loadtxt(iterated / "DSurfTomo_2step.inv", ndmin=2).reshape(NZ, NY, NX, 4)[:NLAY, 1:-1, 1:-1].reshape(-1, 4)
        assert nlines(iterated / name) == NLAY * NCELL and a.shape == (NLAY * NCELL, ncol)
        assert np.array_equal(a[:, :ncol - 5], inv[:, :ncol - 5]), name
        assert (a[:, ncol - 5] > 0).all() and (a[:, ncol - 4] <= a[:, ncol - 5]).all()
    assert np.array_equal(read_mod(res / "MOD_2step"), read_mod(iterated / "MOD_2step"))
    damp = para_damping(files["para.in"])
    vs = read_mod(res / "MOD_2step").astype(np.float32)
    depz = np.array([float(v) for v in (res / "MOD_2step").read_text().splitlines()[0].split()], np.float32)
    pv, sen, nf = ctx.depthkernel(vs, depz, TRC, 2.0)
    assert nf == 0
    w = np.where(pv.reshape(KMAX, NY, NX)[:, 1:-1, 1:-1] != 0, np.float32(1.0) / np.float32(SIGMA_C), np.float32(0.0)).astype(np.float32)
    want_vs = ctx.column_resolution(NX, NY, NLAY, ctx.vs_kernels(vs, sen), w, SMOOTH_VS, damp, depz=depz[:NLAY])
    assert all(len(np.unique(v[1:-1, 1:-1])) > 2 for v in vs[:NLAY])          # (the cells of a layer differ: a wrong order would show)
    lsen = ctx.ti_kernels(vs, depz, TRC, 2.0, ctx.depthkernel(vs, depz, TRC, 2.0, kernels=False)[0])
    want_g = ctx.column_resolution(NX, NY, NLAY, lsen, w, SMOOTH_GCS, damp, depz=depz[:NLAY])
    inv = np.loadtxt(res / "DSurfTomo_2step.inv", ndmin=2).reshape(NZ, NY, NX, 4)[:NLAY, 1:-1, 1:-1].reshape(-1, 4)
    for name, want, ncol in ((NEW[0], want_vs, 9), (NEW[1], want_g, 8)):
        assert nlines(res / name) == NLAY * NCELL
        a = np.loadtxt(res / name, ndmin=2)
        assert a.shape == (NLAY * NCELL, ncol)
        assert np.array_equal(a[:, :3], inv[:, :3]), name             # lon lat depth: the cell order of DSurfTomo_2step.inv
        if ncol == 9:
            assert np.array_equal(a[:, 3], inv[:, 3])
        assert want["n_empty"] == 0 and want["n_failed"] == 0
        for i, k in enumerate(("std_post", "std_noise", "rdiag", "rsum", "width")):
            d = np.abs(a[:, ncol - 5 + i] - want[k].reshape(-1).astype(np.float64)).max()
            print(f"\n[measured] {name} {k}: max |file - python| {d:.3e} (half a printed unit {0.5 * QUANTUM[i]:.0e}), values up to "
                  f"{np.abs(want[k]).max():.4g}")
        for i, k in enumerate(("std_post", "std_noise", "rdiag", "rsum", "width")):
            assert np.abs(a[:, ncol - 5 + i] - want[k].reshape(-1).astype(np.float64)).max() <= 0.5 * QUANTUM[i] * (1 + 1e-6), (name, k)
        assert (a[:, ncol - 5] > 0).all() and (a[:, ncol - 4] <= a[:, ncol - 5]).all()
        tr = want["trace"].reshape(-1) / NLAY
        line = [ln for ln in out.splitlines() if ln.startswith(" resolution " + ("Vs" if ncol == 9 else "Gc/Gs"))]
        assert len(line) == 1, out
        f = line[0].split()
        assert int(f[f.index("cells") + 1]) == NCELL and int(f[f.index("factored") + 1]) == 0
        assert abs(float(f[-2]) - np.sort(tr)[(NCELL + 1) // 2 - 1]) <= 2e-5 and abs(float(f[-1]) - tr.min()) <= 2e-5, line
    log = (res / "para.in_2step.log").read_text()
    assert log.count(" resolution Vs") == 1 and log.count(" resolution Gc/Gs") == 1 and "the regulariser acts on the update" in log


def test_resolution_2_is_refused(tmp_path):
    build()
    files = {**inputs(maxiter=1, iso="F"), **true_maps()}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    out = subprocess.run([DEPTH, "para.in", "2.0", "1.5", "0.02", "2"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert out.returncode != 0 and " ERROR: resolution must be 0 or 1, not 2" in out.stdout.splitlines(), out.stdout + out.stderr
    assert not (tmp_path / "MOD_2step").exists() and not any((tmp_path / n).exists() for n in NEW)
