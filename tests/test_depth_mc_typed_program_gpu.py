"""-m gpu: the program SurfDepthMC_amd with its `types` argument on the 7 x 7 typed case of tests/test_typed_program_gpu.py: the maps
of all four wave types from SurfPhaseMaps_amd sampled together, with the fixed noise level and with one noise scale per type; the
refusals; and Rayleigh-phase input (tests/test_depth_mc_program_gpu.py's) with types 1 against types 0."""
import numpy as np
import pytest

from tests import typed_kernels_ref as T
from tests.test_depth_mc_program_gpu import MC, OUTS, true_knot_files
from tests.test_phase_map_program_gpu import run as run_files
from tests.test_typed_program_gpu import (K, NX, NY, PROF, built, para_text, run, start_model, true_model, typed_case,  # noqa: F401
                                          write_inputs)

pytestmark = pytest.mark.gpu

NSAMPLE, NCHAIN, WIDTH, SIGMA = 200, 16, 0.4, 0.02
NCELL = (NX - 2) * (NY - 2)
TYPES = np.array([[iw, ig] for iw, ig, t in T.SEGMENTS for _ in t])
TYPE_NAMES = ("Rayleigh phase", "Rayleigh group", "Love phase", "Love group")


def mc_args(noise_a0=0, aniso_thin=0, types=1):
    """nsample nchain width sigma_c seed proposal ntemp tmax aniso_thin smooth_gcs sigma_a noise_a0 noise_b0 smooth_vs damp_vs types"""
    return (NSAMPLE, NCHAIN, WIDTH, SIGMA, 1, 1, 1, 16, aniso_thin, 1.0, SIGMA, noise_a0, 1.0, 0, 0, types)


@pytest.fixture(scope="module")
def maps_dir(built, typed_case, tmp_path_factory):
    """the typed data through SurfPhaseMaps_amd, once for the runs below"""
    sv, data = typed_case
    d = write_inputs(tmp_path_factory.mktemp("typed_mc"), para_text(maxiter=3), data)
    run("SurfPhaseMaps_amd", d)
    return d


@pytest.mark.parametrize("noise_a0", [0, 2])
def test_typed_maps_through_the_monte_carlo_program(maps_dir, noise_a0):
    d = maps_dir
    noise = d / "noise_posterior_mc.dat"
    if noise.exists():
        noise.unlink()
    out = run("SurfDepthMC_amd", d, *mc_args(noise_a0))
    assert "Program finishes successfully" in out
    nz = len(PROF)
    post = np.loadtxt(d / "Vs_posterior_mc.dat")
    cells = np.loadtxt(d / "cell_mc.dat")
    curves = np.loadtxt(d / "period_phaseV_mc.dat")
    model = np.loadtxt(d / "DSurfTomo_mc.inv")
    assert post.shape == ((nz - 1) * NCELL, 10) and cells.shape == (NCELL, 5) and model.shape == (nz * NY * NX, 4)
    sampled = cells[:, 2] > 0
    assert sampled.mean() > 0.5
    assert np.isfinite(post[:, :9]).all() and np.isfinite(post[np.tile(sampled, nz - 1), 9]).all()
    assert np.isfinite(cells).all() and np.isfinite(model).all() and (d / "MOD_mc").exists()
    # one curve per virtual period and inner cell, ending in the type's wavetp veltp
    periods = np.concatenate([t for _, _, t in T.SEGMENTS])
    assert curves.shape == (K * NCELL, 6) and np.isfinite(curves).all() and (curves[:, 3] > 2.0).all()
    assert np.allclose(curves[::NCELL, 2], periods) and np.array_equal(curves[:, 4:], np.repeat(TYPES, NCELL, axis=0))
    log = (d / "para.in_mc.log").read_text()
    for name in TYPE_NAMES:
        assert sum(name + ":" in ln and "best model mean |c residual|" in ln for ln in log.splitlines()) == 1, name
    if noise_a0:
        nr = np.loadtxt(noise)
        assert nr.shape == (len(T.SEGMENTS) * NCELL, 8)                       # one block per type
        want = np.repeat([[iw, ig] for iw, ig, _ in T.SEGMENTS], NCELL, axis=0)
        assert np.array_equal(nr[:, 6:], want)
        assert np.array_equal(nr[:, 5].reshape(len(T.SEGMENTS), NCELL)[:, sampled].max(axis=1), [len(t) for _, _, t in T.SEGMENTS])
        lam = nr[:, 2].reshape(len(T.SEGMENTS), NCELL)[:, sampled]
        assert np.isfinite(lam).all() and (lam[nr[:, 5].reshape(len(T.SEGMENTS), NCELL)[:, sampled] > 0] > 0).all()
        assert log.count("median of the mean of lambda over cells") == len(T.SEGMENTS) and "per cell and wave type" in log
    else:
        assert not noise.exists() and "lambda" not in log
    mean = model[:, 3].reshape(nz, NY, NX)
    inner = (slice(0, nz - 1), slice(1, -1), slice(1, -1))
    e0 = np.sqrt(np.mean((start_model()[inner] - true_model()[inner]) ** 2))
    e1 = np.sqrt(np.mean((mean[inner] - true_model()[inner]) ** 2))
    tail = [ln for ln in log.splitlines() if "best model mean |c residual|" in ln]
    print(f"\n[typed Monte-Carlo, noise_a0 {noise_a0}] model error {e0:.4f} -> {e1:.4f} km/s; median std {np.median(post[:, 4]):.4f}\n"
          + "\n".join(tail))
    assert e1 < e0


def test_refusals_name_the_argument_and_the_kernel(maps_dir):
    d = maps_dir
    out = run("SurfDepthMC_amd", d, ok=False)                                 # typed para.in without the argument: as before
    assert "SurfDepthMC_amd" in out and "Monte-Carlo forward model is the" in out and "types = 1" in out
    assert "Program finishes successfully" not in out
    out = run("SurfDepthMC_amd", d, *mc_args(types=0), ok=False)
    assert "types = 1" in out and "Program finishes successfully" not in out
    out = run("SurfDepthMC_amd", d, *mc_args(aniso_thin=5), ok=False)
    assert "Lsen_Gsc" in out and "Rayleigh phase velocities only" in out and "Program finishes successfully" not in out
    out = run("SurfDepthMC_amd", d, *mc_args(types=2), ok=False)
    assert "types must be 0 or 1" in out


def test_rayleigh_phase_input_keeps_every_byte(built, tmp_path):
    """tests/test_depth_mc_program_gpu.py's inputs, the noise scale on: every file in OUTS with types 1 is the one with types 0 (the
    log but for its line of run times)"""
    files, _, _ = true_knot_files()
    got = []
    for types in (0, 1):
        dd = tmp_path / str(types)
        run_files(MC, dd, files, *map(str, (30, 4, 0, 0.01, 7, 1, 2, 8, 0, 1.0, 0.01, 2.0, 1.0, 0, 0, types)))
        names = OUTS + ("noise_posterior_mc.dat",)
        got.append({n: (dd / n).read_bytes() for n in names})
        log = got[-1]["para.in_mc.log"].decode().splitlines()
        assert sum(ln.startswith(" run ") for ln in log) == 1
        got[-1]["para.in_mc.log"] = [ln for ln in log if not ln.startswith(" run ")]
    for n in got[0]:
        assert got[0][n] == got[1][n], n
